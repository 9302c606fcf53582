"""Per-stage timing of the fused Swin window attention: --window 12 (default; pd_window_attn_*_w12) at the shapes of BASELINE configs 3 / 5,
--window 7 (pd_window_attn_*_w7) at the Swin-T stages at 1024^2 bs 2 next to the library path of WindowAttention.forward."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from partdistillation_amd import lib
from partdistillation_amd.functions import window_attention as wa
lib.load()
ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, choices=(12, 7), default=12)
args = ap.parse_args()

def t(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e6


def bench_w7():
    """forward and backward of the kernel and of the library path (the body WindowAttention.forward runs when the kernel does not apply:
    permutes, table gather, bias + mask expanded to [B_, heads, 49, 49] bf16, library SDPA, transpose back; its backward through autograd),
    alternated in one process; the median of 5 windows of 50 calls each.  Then the kernel with the windows-per-workgroup walk forced."""
    import statistics
    import torch.nn.functional as F
    from partdistillation_amd.modeling.backbone import swin

    def med(f):
        return statistics.median(t(f, 50) for _ in range(5))

    def library(qkv, table, index, mask, heads):
        B_, N, C3 = qkv.shape
        C = C3 // 3
        x = qkv.reshape(B_, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
        q, k, v = x[0], x[1], x[2]
        add = swin._TableLookup.apply(table, index).view(N, N, -1).permute(2, 0, 1).unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            add = (add + mask.unsqueeze(1)).unsqueeze(0).expand(B_ // nW, -1, -1, -1, -1).reshape(B_, heads, N, N)
        out = F.scaled_dot_product_attention(q, k, v, attn_mask=add.to(q.dtype), dropout_p=0.0, scale=32 ** -0.5)
        return out.transpose(1, 2).reshape(B_, N, C)

    index = swin.WindowAttention(96, (7, 7), 3).relative_position_index.view(-1).cuda()
    print("Swin-T 1024^2 bs2, window 7 (us per call; lib = library path)")
    for side, heads in ((256, 3), (128, 6), (64, 12), (32, 24)):
        nW = (-(-side // 7)) ** 2
        B_, C = 2 * nW, heads * 32
        qkv = torch.randn(B_, 49, 3 * C, device="cuda").bfloat16().requires_grad_()
        table = (torch.randn(169, heads, device="cuda") * 0.1).requires_grad_()
        go = torch.randn(B_, 49, C, device="cuda").bfloat16()
        for shift in (0, 3):
            reg = wa.shifted_window_regions(side, side, shift, "cuda", window=7) if shift else None
            mask = swin.shifted_window_mask(side, side, 7, shift, "cuda") if shift else None
            q_, t_ = qkv.detach(), table.detach()
            out, lse = wa.fwd_raw_w7(q_, t_, reg, 32 ** -0.5, nW)
            lout = library(qkv, table, index, mask, heads)
            err = (lout.detach().float() - out.float()).abs().max().item()
            fk = lambda: wa.fwd_raw_w7(q_, t_, reg, 32 ** -0.5, nW)
            bk = lambda: wa.bwd_raw_w7(q_, t_, reg, out, go, lse, 32 ** -0.5, nW)
            fl = lambda: library(q_, t_, index, mask, heads)
            bl = lambda: torch.autograd.grad(lout, (qkv, table), go, retain_graph=True)
            r = {k: [] for k in ("fk", "fl", "bk", "bl")}
            for _ in range(5):                                    # alternate the four
                r["fk"].append(t(fk, 50)); r["fl"].append(t(fl, 50)); r["bk"].append(t(bk, 50)); r["bl"].append(t(bl, 50))
            m = {k: statistics.median(v) for k, v in r.items()}
            forced = []
            for ch in (1, 2, 4, 8):
                lib.load().pd_debug_set(b"wattn_chunk", ch)
                forced.append("%d: %.1f / %.1f" % (ch, med(fk), med(bk)))
            lib.load().pd_debug_set(b"wattn_chunk", 0)
            print(f"  heads {heads:2d} B_ {B_:4d} shift {shift}: fwd kernel {m['fk']:7.1f} lib {m['fl']:7.1f} ({m['fl'] / m['fk']:.1f} x)   "
                  f"bwd kernel {m['bk']:7.1f} lib {m['bl']:7.1f} ({m['bl'] / m['bk']:.1f} x)   max |kernel - lib| {err:.3g}")
            print("      windows per workgroup forced, fwd / bwd:", "   ".join(forced))


if args.window == 7:
    bench_w7()
    sys.exit(0)

for name, stages in (("config 3 Swin-B 1024^2 bs2", [(264, 4), (132, 8), (72, 16), (36, 32)]),
                     ("config 5 Swin-L 1280^2 bs2", [(324, 6), (168, 12), (84, 24), (48, 48)])):
    print(name)
    for side, heads in stages:
        nW = (side // 12) ** 2
        B_, C = 2 * nW, heads * 32
        qkv = torch.randn(B_, 144, 3 * C, device="cuda").bfloat16()
        table = torch.randn(529, heads, device="cuda") * 0.1
        go = torch.randn(B_, 144, C, device="cuda").bfloat16()
        for shift in (0, 6):
            reg = wa.shifted_window_regions(side, side, shift, "cuda") if shift else None
            out, lse = wa.fwd_raw(qkv, table, reg, 32 ** -0.5, nW)
            tf = t(lambda: wa.fwd_raw(qkv, table, reg, 32 ** -0.5, nW))
            tb = t(lambda: wa.bwd_raw(qkv, table, reg, out, go, lse, 32 ** -0.5, nW))
            abl = []
            for a in (1, 2, 16, 4, 8, 12, 14, 28, 13):
                lib.load().pd_debug_set(b"wattn_ablate", a)
                abl.append("%d:%.0f" % (a, t(lambda: wa.bwd_raw(qkv, table, reg, out, go, lse, 32 ** -0.5, nW))))
            lib.load().pd_debug_set(b"wattn_ablate", 0)
            print("      ablations", " ".join(abl))
            units = B_ * heads
            gf = units * 4 * 144 * 144 * 32 / 1e9          # QK^T + PV forward flops
            print(f"  grid {side}^2 heads {heads:2d} shift {shift}: units {units:6d}  fwd {tf:7.1f} us ({gf / tf * 1e-3 * 1e3:6.1f} TF)"
                  f"  bwd {tb:7.1f} us ({2.5 * gf / tb * 1e-3 * 1e3:6.1f} TF)  qkv {qkv.numel() * 2 / 1e6:.0f} MB")
