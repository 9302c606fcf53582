"""The ctypes binding (partdistillation_amd/lib.py) is derived from include/*.h.  Here the C++ compiler judges the derived objects
against the headers (prototypes, struct layouts, constants), the awkward declarations are pinned by hand, the reader's refusals are
exercised, and the exported, declared and recordable sets are compared.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from partdistillation_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, F, D, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_char_p
CODE = {id(P): "p", id(S): "p", id(F): "f", id(D): "d", id(L): "l", id(I): "i", id(None): "v"}


def _code(name):
    """return type first, then the parameters: p pointer, f float, d double, l 8-byte integer, i 4-byte integer, v void"""
    res, args = lib.SIGNATURES[name]
    return "".join(CODE[id(t)] for t in [res] + args)


# ---------------------------------------------------------------------------------------------- 1. the compiler is the oracle
PRELUDE = r"""
#include <cstddef>
#include <cstdint>
#include <type_traits>
template <class T> constexpr char code()
{
  if constexpr (std::is_void_v<T>) return 'v';
  else return std::is_pointer_v<T> ? 'p' : std::is_same_v<T, float> ? 'f' : std::is_same_v<T, double> ? 'd'
            : std::is_integral_v<T> && sizeof(T) == 8 ? 'l' : std::is_integral_v<T> && sizeof(T) == 4 ? 'i' : '?';
}
template <class R, class... A> constexpr bool same(R (*)(A...), const char *s)
{
  const char c[] = {code<R>(), code<A>()..., 0};
  for (size_t i = 0; i < sizeof(c); ++i)          // the terminating 0 is compared too: equal lengths
    if (c[i] != s[i]) return false;
  return true;
}
"""


def test_the_compiler_agrees_with_every_derived_prototype_struct_and_constant(tmp_path):
    cxx = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("g++") or shutil.which("c++"))
    assert cxx, "no C++ compiler: the library cannot be built either"
    head = [PRELUDE] + [f'#include "{h}"' for h in sorted(os.listdir(lib.INCLUDE)) if h.endswith(".h")]
    tu = list(head)
    for name in sorted(lib.SIGNATURES):
        tu.append(f'static_assert(same(&{name}, "{_code(name)}"), "{name}: binding {_code(name)}");')
    for name, st in sorted(lib._STRUCTS.items()):
        tu.append(f'static_assert(sizeof({name}) == {ctypes.sizeof(st)} && alignof({name}) == {ctypes.alignment(st)}, "{name}");')
        for f, _ in st._fields_:
            d = getattr(st, f)
            tu.append(f'static_assert(offsetof({name}, {f}) == {d.offset} && sizeof({name}::{f}) == {d.size}, "{name}.{f}");')
    for name, v in sorted(lib._CONSTS.items()):
        tu.append(f'static_assert(({name}) == {v}, "{name}");')
    assert len(lib.SIGNATURES) >= 205 and len(lib._STRUCTS) >= 21 and len(lib._CONSTS) >= 29           # (213 before the eight three-plane forward entry points and queries went)
    src = tmp_path / "abi.cpp"
    src.write_text("\n".join(tu) + "\n")
    out = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", lib.INCLUDE, str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    # the oracle itself: a wrong code, a wrong offset and a wrong constant are each refused
    for bad in ('static_assert(same(&pd_adamw_clipped, "ippppliffffdipdpp"), "float for double");',
                'static_assert(offsetof(PdCmd, kind) == 8 + 8 * 32, "the old PD_CMD_MAX_ARGS");',
                'static_assert((PD_ABI_VERSION) == 48, "stale version");'):
        src.write_text("\n".join(head + [bad]) + "\n")
        out = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", lib.INCLUDE, str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode != 0 and "static assertion failed" in out.stdout.replace("static_assert failed", "static assertion failed"), bad


# ---------------------------------------------------------------------------------------------- 2. pinned by hand
def test_awkward_prototypes_are_what_the_headers_say():
    sig = lib.SIGNATURES
    assert sig["pd_last_error"] == (S, []) and sig["pd_last_error"][0] is ctypes.c_char_p                 # const char *pd_last_error(void)
    assert sig["pd_stem_wgrad_workspace_floats"] == (L, []) and sig["pd_abi_version"] == (I, []) and sig["pd_dec_split"] == (I, [])
    assert sig["pd_adamw_clipped"] == (I, [P] * 4 + [L, I] + [D] * 5 + [I, P, D, P, P])                   # lr, beta1, beta2, eps, weight_decay ... max_norm
    assert sig["pd_matcher_costs"] == (I, [P, I, P] + [L] * 3 + [P] * 3 + [I] * 6 + [F] * 3 + [P])
    assert sig["pd_dcrf_prepare"] == (I, [P, P] + [I] * 3 + [D] * 4 + [P] * 5)
    assert sig["pd_window_attn_fwd_w7"] == (I, [P] * 6 + [I] * 3 + [F, P])                                # the scale, then the stream
    assert sig["pd_rle_sample_groups_u8"][1][11] is I and len(sig["pd_rle_sample_groups_u8"][1]) == 16
    assert sig["pd_cmd_fn_index"] == (I, [S]) and sig["pd_debug_set"] == (I, [S, I]) and sig["pd_debug_get"] == (I, [S, P])
    assert sig["pd_igemm_bf16_time"] == sig["pd_wgrad_bf16_time"] == (I, [P, P, L, I, P, P])
    assert sig["pd_dbg_set_wgrad_xcd"] == (None, [I])
    for res, args in sig.values():                                  # the singletons cmdbuf._record tests with `is`
        assert all(any(t is k for k in (P, I, L, F, D, S)) for t in args) and any(res is k for k in (P, I, L, S, None))


def test_awkward_structs_and_constants_are_what_the_headers_say():
    cmd = lib.struct("PdCmd")
    assert [f for f, _ in cmd._fields_] == ["fn", "nargs", "a", "kind"]
    assert ctypes.sizeof(cmd) == 8 + 8 * 48 + 2 * 48 and cmd.kind.offset == 8 + 8 * 48 and cmd.a.offset == 8
    assert cmd._fields_[2][1]._length_ == 48 and cmd._fields_[2][1]._type_ is ctypes.c_uint64
    assert cmd._fields_[3][1]._length_ == 48 and cmd._fields_[3][1]._type_ is ctypes.c_int16
    tr = lib.struct("PdTransposeProblem")                           # the anonymous `typedef struct { ... } Name;` form
    assert tr._fields_ == [("src", P), ("dst", P), ("src_batch_stride", L), ("src_row_stride", L),
                           ("batch", I), ("rows", I), ("cols", I), ("reserved", I)] and ctypes.sizeof(tr) == 48
    ig = lib.struct("PdIgemm")
    assert [f for f, _ in ig._fields_][-1] == "out_col_slab" and ctypes.sizeof(ig) == 9 * 8 + 16 * 4 and ig.batch.offset == 72
    sw = lib.struct("PdSgemmWgradDesc")                             # `const void *dY, *X;`: several declarators on one line
    assert [f for f, _ in sw._fields_][:4] == ["dY", "X", "dW", "dB"] and all(t is P for _, t in sw._fields_[:4])
    assert lib.struct("PdIgemm") is lib.struct("PdIgemm")
    assert (lib.const("PD_CMD_MAX_ARGS"), lib.const("PD_CMD_LITERAL"), lib.const("PD_CMD_STREAM")) == (48, -1, -2)
    assert lib.const("PD_SAMPLE_GROUPS_MAX") == 1 << 20 and lib.const("PD_UNCERTAIN_MAX_K") == 40960 and lib.const("PD_WGRAD_SEQ_MAX") == 8
    assert "PD_MSDA_H" not in lib._CONSTS                            # an include guard is no constant
    from partdistillation_amd import cmdbuf
    from partdistillation_amd.functions import igemm, mx8
    assert cmdbuf.PdCmd is cmd and igemm.PdIgemm is ig and mx8.PdMx8Gemm is lib.struct("PdMx8Gemm")
    assert (cmdbuf.MAX_ARGS, cmdbuf.LITERAL, cmdbuf.STREAM, igemm.WGRAD_SEQ_MAX) == (48, -1, -2, 8)


# ---------------------------------------------------------------------------------------------- 3. what the reader refuses
GOOD = "#include <stdint.h>\n#define PD_N (1 << 3)\ntypedef struct { const float *a, *b; int32_t k, n; uint8_t tag[PD_N]; } PdT;\nint64_t pd_ok(const PdT *t, float s, void *stream);\n"


def _read(tmp_path, text):
    (tmp_path / "pd_x.h").write_text(text)
    return lib.read_headers(str(tmp_path))


def test_reader_reads_the_subset_and_ignores_comments(tmp_path):
    sigs, structs, consts = _read(tmp_path, GOOD + "/* int pd_fake(int); */\n// int pd_fake2(int);\nenum { PD_A = 0 };\n")
    assert sigs == {"pd_ok": (L, [P, F, P])} and consts == {"PD_N": 8}
    t = structs["PdT"]
    assert [f for f, _ in t._fields_] == ["a", "b", "k", "n", "tag"] and ctypes.sizeof(t) == 32 and t.tag.offset == 24 and t.tag.size == 8


@pytest.mark.parametrize("text,offender", [
    ("int pd_bad(unsigned flags, void *stream);\n", "unsigned flags"),                       # unknown parameter type
    ("int pd_bad(size_t n);\n", "size_t n"),
    ("long pd_bad(void);\n", "long"),                                                        # unknown return type
    ("typedef struct PdO { int32_t a; struct PdIn { int32_t b; } in; } PdO;\n", "struct PdIn"),   # nested struct field
    ("typedef struct PdO { int32_t a; PdT t; } PdO;\n", "PdT t"),                            # a struct by value
    ("typedef struct PdO { long a; } PdO;\n", "long a"),
    ("typedef struct PdO { int32_t a[PD_MISSING]; } PdO;\n", "PD_MISSING"),
    ("#define PD_X 1.5f\n", "1.5f"),                                                         # non-integer constants
    ("#define PD_X \"text\"\n", "text"),
    ("#define PD_X 0x10\n", "0x10"),
    ("#define PD_X (1 << 3\n", "(1 << 3"),
    ("#define PD_X(a) (a)\n", "PD_X(a)"),
    ("#if PD_N > 4\nint pd_more(void);\n#endif\n", "#if PD_N > 4"),
    ("int pd_bad(int a)\n", "pd_bad"),                                                       # no semicolon: runs into the end of the file
    ("static inline int helper(int a) { return a; }\n", "helper"),
])
def test_reader_refuses_what_it_cannot_classify(tmp_path, text, offender):
    with pytest.raises(lib.PdHipError) as e:
        _read(tmp_path, GOOD + text)
    assert "pd_x.h" in str(e.value) and offender in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------- 4. sets
# the recordable entry points (kTable of csrc/cmdbuf.hip): which calls a recording captures is behaviour, so a change here is a
# decision (tools/gen_cmdbuf_table.py), never a side effect.  144 as of the commit that introduced the derived binding; 137 since the
# seven three-plane forward / input-gradient entry points (GEMM, pre-split, ReLU-bit and 3 x 3 convolution forms) were retired
RECORDABLE = """
pd_adamw_clipped pd_adamw_clipped_shadow pd_add_layernorm_bwd pd_add_layernorm_bwd_amax pd_add_layernorm_fwd pd_add_layernorm_fwd_amax
pd_add_rows_amax_f32 pd_affine_act_bwd2_bf16 pd_affine_act_bwd_bf16 pd_affine_act_fwd_bf16 pd_attn_bwd_d32 pd_attn_bwd_d32_ld
pd_attn_fwd_d32 pd_attn_fwd_d32_ld pd_attn_mask_u8 pd_cast_bf16_f32_amax pd_colsum_acc pd_conv3x3_nhwc_f16x2 pd_conv3x3_wgrad_nhwc_f16x2
pd_conv_bf16_dgrad pd_conv_bf16_fwd pd_conv_bf16_wgrad pd_conv_bf16_wgrad_grouped pd_copy_segments pd_dec_bwd_a pd_dec_bwd_b pd_dec_fwd_a
pd_dec_fwd_b pd_dec_pack_grouped pd_decoder_head_bf16 pd_filter_transpose_grouped pd_gemm_tn_f16x2 pd_gemm_tn_f16x2_bf16out pd_gemm_tn_f32
pd_gemm_wgrad_acc_f16x2_ws pd_gemm_wgrad_acc_f32 pd_gemm_wgrad_acc_f32x3 pd_gemm_wgrad_acc_f32x3_ws pd_gemm_wgrad_f16x2_grouped
pd_gemm_wgrad_f32 pd_gemm_wgrad_f32x3_grouped pd_gn_coeffs_bwd pd_gn_coeffs_fwd pd_igemm_bf16 pd_igemm_bf16_seq pd_kmeans_assign
pd_kmeans_assign_bounded pd_kmeans_assign_partial pd_kmeans_reduce pd_kmeans_reduce_update pd_kmeans_reduce_update_shift pd_kmeans_update
pd_layernorm_rows_f32_bwd pd_layernorm_rows_f32_fwd pd_loss_vectors_bwd pd_loss_vectors_fwd pd_lsa_batched pd_mask_assign
pd_mask_point_losses_bwd pd_mask_point_losses_fwd pd_match_point_logits pd_matcher_costs pd_matcher_point_terms pd_maxpool3s2_bwd_bf16
pd_maxpool3s2_fwd_bf16 pd_mem_prep_bwd pd_mem_prep_fwd pd_memcpy_d2d_async pd_memset_async pd_msda_backward pd_msda_forward
pd_msda_forward_amax pd_msda_fused_backward pd_msda_fused_forward pd_msda_prep_bwd pd_msda_prep_bwd_amax pd_msda_prep_fwd
pd_multi_gather_sumsq pd_mx8_gemm pd_mx8_quantize_bf16 pd_mx8_quantize_grouped pd_nc_affine2_amax_f32 pd_nc_affine2_f32
pd_nc_affine_amax_f32 pd_nc_affine_f32 pd_nc_sums_f32 pd_normalize_u8_nhwc pd_pair_logits_bwd_rows pd_pair_logits_bwd_tok pd_pair_logits_fwd
pd_point_sample_nhwc_f32 pd_point_sample_nhwc_f32_bf16 pd_point_sample_planar_bwd_f32 pd_point_sample_planar_f32 pd_point_sample_u8
pd_poly_crossings_i32 pd_relu_bwd_colsum pd_resample_cols_canvas_u8 pd_resample_rows_u8 pd_resize_bilinear_nhwc_f32
pd_rle_sample_groups_canvas_u8 pd_rle_sample_groups_u8 pd_rle_sample_u8 pd_row_amax_f32 pd_scores_argmax_u8 pd_sgemm_nn_bf16
pd_sgemm_nn_splitn_bf16 pd_sgemm_tn_batched_bf16 pd_sgemm_tn_bf16 pd_sgemm_tn_multi_bf16 pd_sgemm_tn_splitk_bf16 pd_sgemm_wgrad_bf16
pd_sgemm_wgrad_grouped_bf16 pd_sgemm_wgrad_split_bf16 pd_skinny_linear_bwd pd_skinny_linear_fwd pd_stem7x7_fwd pd_stem7x7_wgrad
pd_sum3_sum2_f32 pd_sumsq_accumulate pd_swin_ln_bwd pd_swin_ln_fwd pd_swin_merge_ln_bwd pd_swin_merge_ln_fwd pd_swin_tail_ln_bwd
pd_swin_tail_ln_fwd pd_transpose_batched_f32 pd_uncertain_points pd_upsample2x_bwd_nhwc_f32 pd_upsample_add_amax_nhwc_f32
pd_upsample_add_nhwc_f32 pd_wgrad_bf16 pd_wgrad_bf16_seq pd_window_attn_bwd_w12 pd_window_attn_bwd_w7 pd_window_attn_fwd_w12
pd_window_attn_fwd_w7
""".split()


def test_exported_declared_and_recordable_sets():
    lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW" and ln.split()[2].startswith("pd_")}
    assert exported == set(lib.SIGNATURES), (sorted(exported - set(lib.SIGNATURES)), sorted(set(lib.SIGNATURES) - exported))
    so = lib.load()
    assert len(RECORDABLE) == len(set(RECORDABLE)) == 137
    recordable = {n for n in lib.SIGNATURES if so.pd_cmd_fn_index(n.encode()) >= 0}
    assert recordable == set(RECORDABLE), (sorted(recordable - set(RECORDABLE)), sorted(set(RECORDABLE) - recordable))
    for n in RECORDABLE:                                             # Thunk<&f>::nargs, from the real prototype, against the derived argtypes
        assert so.pd_cmd_fn_nargs(so.pd_cmd_fn_index(n.encode())) == len(lib.SIGNATURES[n][1]) <= lib.const("PD_CMD_MAX_ARGS"), n
        assert lib.SIGNATURES[n][0] is I and lib.SIGNATURES[n][1][-1] is P, n      # returns a status, ends with the stream
    assert so.pd_cmd_fn_index(b"pd_no_such_function") == -1


# ---------------------------------------------------------------------------------------------- 5. one ABI version
def test_the_abi_version_is_written_once():
    assert lib.ABI_VERSION == lib.const("PD_ABI_VERSION") == lib.load().pd_abi_version()
    v, hits = str(lib.ABI_VERSION), []
    for top in ("include", "partdistillation_amd", "tools", "oracle", "tests", "."):
        for dirpath, dirs, files in os.walk(os.path.join(ROOT, top)):
            if top == ".":
                dirs[:] = []
            dirs[:] = [d for d in dirs if not d.startswith((".", "_")) and d != "golden"]
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".inc", ".cpp", ".c", ".sh", ".md")) and os.path.join(dirpath, f) != os.path.abspath(__file__):
                    for ln in open(os.path.join(dirpath, f), errors="replace"):
                        if re.search(r"(?i)abi[ _]?version", ln) and re.search(rf"\b{v}\b", ln):
                            hits.append((os.path.relpath(os.path.join(dirpath, f), ROOT), ln.strip()))
    assert hits == [(os.path.join("include", "pd_msda.h"), f"#define PD_ABI_VERSION {v}")], hits
