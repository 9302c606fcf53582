"""Regenerates the table of recordable entry points inside partdistillation_amd/csrc/cmdbuf.hip from include/*.h, as the binding reads them
(partdistillation_amd.lib.read_headers): every function that returns `int` except the host-only queries and the development knobs.
Run after adding a C-ABI function that a recorded region calls:  python tools/gen_cmdbuf_table.py"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from partdistillation_amd import lib
SKIP = {"pd_abi_version", "pd_conv_bf16_supported", "pd_igemm_bf16_supported", "pd_gemm_wgrad_f16x2_takes_wide_tiles",
        "pd_point_sample_planar_bwd_needs_zero", "pd_point_sample_planar_bwd_needs_zero_n", "pd_msda_backward_last_gate", "pd_msda_fused_supported", "pd_gemm_tn_f16x2_which", "pd_debug_set",
        "pd_cmd_replay", "pd_cmd_fn_index", "pd_cmd_fn_nargs", "pd_igemm_bf16_time", "pd_mx8_gemm_supported", "pd_debug_get", "pd_wgrad_bf16_time", "pd_debug_read_kpc_trace"}
# entry points of evaluation, label export and pseudo-label refinement (and two host-only queries): no recorded region calls them and
# the table has never held them; cmdbuf.hip does not include pd_assign.h, pd_dcrf.h, pd_eval.h, pd_pparts.h or pd_rle.h.  Move a name out of here,
# and add its #include there, when a recorded region starts to call it.
UNRECORDED = {"pd_assign_histogram", "pd_mask_assign_resized", "pd_masks_resize_u8", "pd_scores_argmax_resized_u8", "pd_dec_split",
              "pd_pair_assign_resized",
              "pd_dcrf_argmax", "pd_dcrf_bilateral_update", "pd_dcrf_prepare", "pd_dcrf_spatial_message",
              "pd_eval_confusion_grouped", "pd_eval_intersect_grouped", "pd_eval_pack_grouped", "pd_eval_recall_grouped",
              "pd_rle_decode", "pd_rle_plane_runs", "pd_rle_seg_rows",
              "pd_pp_decode_uids", "pd_rle_masked_label_runs"}
names = sorted(n for n, (res, _) in lib.SIGNATURES.items() if res is ctypes.c_int and n not in SKIP | UNRECORDED)
p = os.path.join(ROOT, "partdistillation_amd", "csrc", "cmdbuf.hip")
s = open(p).read()
a, b = s.index("const Entry kTable[] = {\n") + len("const Entry kTable[] = {\n"), s.index("};\nconstexpr int kCount")
s = s[:a] + "".join(f"  PD_E({n}),\n" for n in names) + s[b:]
open(p, "w").write(s)
print(len(names), "recordable entry points")
