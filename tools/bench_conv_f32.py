#!/usr/bin/env python
"""The fp32 backbone convolutions of include/pd_conv_f32.h next to the library's (F.conv2d / aten.convolution_backward in fp32), layer class
by layer class of R50 at 1024^2, batch 2: forward (with the frozen-BN affine and ReLU on both sides: the library side as the folded filter +
bias + relu_ of resnet._conv_bn_act), input gradient, filter gradient.  Device events around `--iters` launches after `--warmup` ones, both
routes warmed before either is timed and timed alternately, median of `--rounds` rounds.

--step: a config-2 TrainStep (R50 Mask2Former, 1024^2, batch 2) with AMP off, the switch of modeling/backbone/resnet.py off and on in the same
process, alternating.

    python tools/bench_conv_f32.py [--step] [--out bench_conv_f32.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"

# (name, input side, ci, co, k, stride) at a 1024^2 image: the stem's output is 512^2, the max pooling's 256^2
LAYERS = [
    ("res2 1x1 s1  64->64", 256, 64, 64, 1, 1), ("res2 1x1 s1  64->256", 256, 64, 256, 1, 1), ("res2 1x1 s1 256->64", 256, 256, 64, 1, 1),
    ("res2 3x3 s1  64", 256, 64, 64, 3, 1),
    ("res3 1x1 s1 256->128", 256, 256, 128, 1, 1), ("res3 1x1 s1 128->512", 128, 128, 512, 1, 1), ("res3 1x1 s2 256->512", 256, 256, 512, 1, 2),
    ("res3 3x3 s2 128", 256, 128, 128, 3, 2), ("res3 3x3 s1 128", 128, 128, 128, 3, 1),
    ("res4 1x1 s1 512->256", 128, 512, 256, 1, 1), ("res4 1x1 s1 256->1024", 64, 256, 1024, 1, 1), ("res4 1x1 s2 512->1024", 128, 512, 1024, 1, 2),
    ("res4 3x3 s2 256", 128, 256, 256, 3, 2), ("res4 3x3 s1 256", 64, 256, 256, 3, 1),
    ("res5 1x1 s1 1024->512", 64, 1024, 512, 1, 1), ("res5 1x1 s1 512->2048", 32, 512, 2048, 1, 1), ("res5 1x1 s2 1024->2048", 64, 1024, 2048, 1, 2),
    ("res5 3x3 s2 512", 64, 512, 512, 3, 2), ("res5 3x3 s1 512", 32, 512, 512, 3, 1),
]


def timed(fns, warmup, iters, rounds):
    """fns: {route: callable} -> {route: median ms per call}; every route warmed first, then timed in alternation"""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / iters)
    return {k: statistics.median(v) for k, v in ms.items()}


def layer(name, B, side, ci, co, k, s, args):
    from partdistillation_amd import lib
    L, st = lib.load(), lib.current_stream
    stem = ci == 3
    p = k // 2
    ho = (side + 2 * p - k) // s + 1
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((B, ci, side, side), device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    w = (torch.randn((co, ci, k, k), device=DEV, generator=g) / (ci * k * k) ** 0.5).contiguous(memory_format=torch.channels_last)
    dz = torch.randn((B, co, ho, ho), device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    scale, bias = torch.rand(co, device=DEV, generator=g) + 0.5, torch.randn(co, device=DEV, generator=g)
    wk = w.permute(0, 2, 3, 1).contiguous()
    wt = w.permute(1, 2, 3, 0).contiguous()
    y, dx, dw = torch.empty_like(dz), torch.empty_like(x), torch.empty_like(wk)
    ws = torch.empty(int(L.pd_conv_f32_wgrad_workspace_floats(B, ho, ho, ci, co, k)), dtype=torch.float32, device=DEV)
    wf = w * scale.view(-1, 1, 1, 1)
    chk = lib.check
    if stem:
        own = {"fwd": lambda: chk(L.pd_stem7x7_f32_fwd(x.data_ptr(), wk.data_ptr(), scale.data_ptr(), bias.data_ptr(), y.data_ptr(), B, side, side,
                                                       ho, ho, co, 1, st())),
               "wgrad": lambda: chk(L.pd_stem7x7_f32_wgrad(dz.data_ptr(), x.data_ptr(), scale.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), B,
                                                           side, side, ho, ho, co, st()))}
    else:
        own = {"fwd": lambda: chk(L.pd_conv_f32_fwd(x.data_ptr(), wk.data_ptr(), scale.data_ptr(), bias.data_ptr(), None, y.data_ptr(), B, side, side,
                                                    ci, ho, ho, co, k, s, p, 1, st())),
               "dgrad": lambda: chk(L.pd_conv_f32_dgrad(dz.data_ptr(), wt.data_ptr(), None, dx.data_ptr(), B, side, side, ci, ho, ho, co, k, s, p, st())),
               "wgrad": lambda: chk(L.pd_conv_f32_wgrad(dz.data_ptr(), x.data_ptr(), scale.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), B,
                                                        side, side, ci, ho, ho, co, k, s, p, st()))}
    cb = torch.ops.aten.convolution_backward
    bw = lambda mask: cb(dz, x, w, None, [s, s], [p, p], [1, 1], False, [0, 0], 1, mask)
    libf = {"fwd": lambda: F.relu_(F.conv2d(x, wf, bias, s, p)), "dgrad": lambda: bw([True, False, False]), "wgrad": lambda: bw([False, True, False])}
    flop = 2.0 * B * ho * ho * co * ci * k * k
    row = {"layer": name, "gflop": flop / 1e9}
    for op in own:
        t = timed({"own": own[op], "lib": libf[op]}, args.warmup, args.iters, args.rounds)
        row[op] = {"own_ms": t["own"], "lib_ms": t["lib"], "own_tflops": flop / t["own"] / 1e9, "lib_tflops": flop / t["lib"] / 1e9}
    return row


def step_times(args):
    from partdistillation_amd.config import setup_cfg
    from partdistillation_amd.engine.synthetic import make_batch
    from partdistillation_amd.engine.trainer import TrainStep
    from partdistillation_amd.modeling.backbone import resnet
    cfg = setup_cfg(os.path.join(ROOT, "partdistillation_amd", "configs", "proposal_learning", "r50_mask2former.yaml"),
                    ["INPUT.IMAGE_SIZE", str(args.size), "SOLVER.AMP.ENABLED", "False"])
    torch.manual_seed(0)
    step = TrainStep(cfg)
    batches = [make_batch(args.batch, args.size, seed=1234 + 1000 * i, device=DEV) for i in range(2)]
    n = [0]

    def run(on):
        def f():
            resnet.OWN_FP32 = on
            step(batches[n[0] % 2])
            n[0] += 1
        return f
    t = timed({"switch off": run(False), "switch on": run(True)}, args.step_warmup, args.step_iters, args.rounds)
    resnet.OWN_FP32 = False
    return {"size": args.size, "batch": args.batch, "amp": False, "off_ms": t["switch off"], "on_ms": t["switch on"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time a config-2 TrainStep with AMP off, switch off and on")
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the figures to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv_f32.py needs a GPU: a time taken anywhere else says nothing")
    f = args.size / 1024.0
    rows = [layer("stem 7x7 s2 3->64", args.batch, args.size, 3, 64, 7, 2, args)]
    rows += [layer(n, args.batch, max(1, int(side * f)), ci, co, k, s, args) for n, side, ci, co, k, s in LAYERS]
    print("| layer | GFLOP | fwd own / lib ms | dgrad own / lib ms | wgrad own / lib ms | own TFLOP/s fwd / dgrad / wgrad |")
    print("|---|---|---|---|---|---|")
    cell = lambda r, op: "%.3f / %.3f" % (r[op]["own_ms"], r[op]["lib_ms"]) if op in r else "-"
    for r in rows:
        tf = " / ".join("%.1f" % r[op]["own_tflops"] if op in r else "-" for op in ("fwd", "dgrad", "wgrad"))
        print("| %s | %.2f | %s | %s | %s | %s |" % (r["layer"], r["gflop"], cell(r, "fwd"), cell(r, "dgrad"), cell(r, "wgrad"), tf))
    result = {"layers": rows}
    if args.step:
        result["step"] = step_times(args)
        print("TrainStep %d^2 batch %d AMP off: switch off %.1f ms, switch on %.1f ms" % (args.size, args.batch, result["step"]["off_ms"],
                                                                                         result["step"]["on_ms"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
