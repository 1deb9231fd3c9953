"""ctypes binding of the C ABI in include/fhe_hip.h (libfhe_hip.so, built for gfx950).

This is plumbing for tests and bench.py: the product is the C-ABI library itself.  There is NO CPU
fallback: constructing `Lib()` raises if the HIP library has not been built, and every call raises
`FheError` with the library's message if the device is unusable.

Host-side mirror of the reference surface: `Context` ~ ILDCRTParams + twiddle cache, `Tower` ~
lbcrypto::DCRTPoly (src/core/include/lattice/hal/default/dcrtpoly.h:59-398) holding a batch of
device-resident towers, with the reference's method names (SwitchFormat, Plus, Minus, Times,
AutomorphismTransform, ApproxSwitchCRTBasis ...).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SO = os.path.join(_HERE, "csrc", "libfhe_hip.so")

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
vp = C.c_void_p
u32 = C.c_uint32
u64 = C.c_uint64
EVALUATION, COEFFICIENT = 0, 1  # lbcrypto::Format (src/core/include/utils/inttypes.h:65)


class FheError(RuntimeError):
    pass


def _np_u32(a):
    if a is None:
        return None, None
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
    return arr, arr.ctypes.data_as(u32p)


class Lib:
    """Loads libfhe_hip.so (or an explicitly given build, e.g. the test-only lane emulator)."""

    def __init__(self, path=None, may_lack=()):
        """may_lack: name prefixes of entry points that `path` — an older build kept as a baseline by a measuring tool — is known not to
        have; those stay unbound, every other missing symbol is an error as always"""
        path = path or os.environ.get("FHE_HIP_LIB") or DEFAULT_SO
        if not os.path.exists(path):
            raise FheError(
                f"{path} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback.")
        self.path = path
        L = self.L = C.CDLL(path)

        def S(name, res, args):
            try:
                f = getattr(L, name)
            except AttributeError:
                if name.startswith(tuple(may_lack)) and may_lack:
                    return
                raise
            f.restype, f.argtypes = res, args

        S("fhe_last_error", C.c_char_p, [])
        S("fhe_version", C.c_char_p, [])
        S("fhe_device_count", C.c_int, [])
        S("fhe_ctx_create", C.c_int, [u32, u32, u64p, u64p, C.c_int, C.POINTER(vp)])
        S("fhe_ctx_destroy", None, [vp])
        S("fhe_ctx_logn", u32, [vp])
        S("fhe_ctx_limbs", u32, [vp])
        S("fhe_ctx_device", C.c_int, [vp])
        S("fhe_malloc", C.c_int, [vp, C.c_size_t, C.POINTER(vp)])
        S("fhe_free", C.c_int, [vp, vp])
        for n in ("fhe_memcpy_h2d", "fhe_memcpy_d2h", "fhe_memcpy_d2d"):
            S(n, C.c_int, [vp, vp, vp, C.c_size_t, vp])
        S("fhe_stream_sync", C.c_int, [vp, vp])
        S("fhe_stream_create", C.c_int, [vp, C.POINTER(vp)])
        S("fhe_stream_destroy", C.c_int, [vp, vp])
        S("fhe_stream_wait", C.c_int, [vp, vp, vp])
        S("fhe_memset_zero", C.c_int, [vp, vp, C.c_size_t, vp])
        S("fhe_checksum", C.c_int, [vp, vp, u32, vp, vp])
        S("fhe_graph_begin", C.c_int, [vp, vp])
        S("fhe_graph_end", C.c_int, [vp, vp, C.POINTER(vp)])
        S("fhe_graph_launch", C.c_int, [vp, vp, vp])
        S("fhe_graph_destroy", None, [vp])
        S("fhe_ntt_fwd", C.c_int, [vp, vp, u32p, u32, u32, vp])
        S("fhe_ntt_inv", C.c_int, [vp, vp, u32p, u32, u32, vp])
        S("fhe_ntt_fwd_oop", C.c_int, [vp, vp, vp, u32p, u32, u32, vp])
        S("fhe_ntt_inv_oop", C.c_int, [vp, vp, vp, u32p, u32, u32, vp])
        for n in ("fhe_add", "fhe_sub", "fhe_mul", "fhe_mul_add"):
            S(n, C.c_int, [vp, vp, vp, vp, u32p, u32, u32, vp])
        S("fhe_neg", C.c_int, [vp, vp, vp, u32p, u32, u32, vp])
        S("fhe_mul_const", C.c_int, [vp, vp, vp, u64p, u32p, u32, u32, vp])
        S("fhe_mult_acc", C.c_int, [vp, vp, vp, u64p, u32p, u32, u32, vp])
        S("fhe_times_q_over_t", C.c_int, [vp, vp, vp, u64, u64, u64p, u32p, u32, u32, vp])
        S("fhe_mod_switch_round", C.c_int, [vp, vp, u64, u64, vp, C.c_size_t, vp])
        S("fhe_inner_product", C.c_int, [vp, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), u32p, u32p, u32, u32, vp, vp, vp])
        S("fhe_add_const", C.c_int, [vp, vp, vp, u64p, u32p, u32, u32, C.c_int, vp])
        S("fhe_sub_const", C.c_int, [vp, vp, vp, u64p, u32p, u32, u32, vp])
        S("fhe_poly_mul_workspace_bytes", C.c_size_t, [vp, u32, u32])
        S("fhe_poly_mul", C.c_int, [vp, vp, vp, vp, u32p, u32, u32, vp, C.c_size_t, vp])
        S("fhe_tensor_square", C.c_int, [vp, vp, vp, vp, vp, vp, u32p, u32, u32, vp])
        S("fhe_mod_up", C.c_int, [vp, vp, C.c_int, vp, u32, vp, C.c_size_t, vp])
        S("fhe_expand_crt_basis_ql_hat", C.c_int, [vp, vp, u32, u64p, u32p, u32, u32, vp, vp])
        S("fhe_tensor", C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, u32p, u32, u32, vp])
        S("fhe_automorph", C.c_int, [vp, vp, vp, u32, C.c_int, u32p, u32, u32, vp])
        S("fhe_switch_modulus", C.c_int, [vp, vp, u32p, u32, vp, u32, u32, u32, u32, vp])
        S("fhe_crt_decompose_towers", u32, [vp, u32p, u32, u32])
        S("fhe_crt_decompose", C.c_int, [vp, vp, u32p, u32, u32, vp, vp])
        S("fhe_event_create", C.c_int, [vp, C.POINTER(vp)])
        S("fhe_event_record", C.c_int, [vp, vp, vp])
        S("fhe_stream_wait_event", C.c_int, [vp, vp, vp])
        S("fhe_event_destroy", C.c_int, [vp, vp])
        S("fhe_sample_uniform", C.c_int, [vp, vp, u32p, u32, u32, C.c_uint64, u32, vp])
        S("fhe_sample_gaussian", C.c_int, [vp, vp, u32p, u32, u32, C.c_double, C.c_uint64, u32, vp])
        S("fhe_sample_ternary", C.c_int, [vp, vp, u32p, u32, u32, C.c_uint64, u32, vp])
        S("fhe_blake2xb_stream", C.c_int, [vp, vp, u64, u32p, u64, vp])
        S("fhe_sample_uniform_blake2", C.c_int, [vp, vp, u32p, u32, u32, u32p, u64, vp])
        S("fhe_sample_gaussian_blake2", C.c_int, [vp, vp, u32p, u32, u32, C.c_double, u32p, u64, vp])
        S("fhe_sample_ternary_blake2", C.c_int, [vp, vp, u32p, u32, u32, u32p, u64, vp])
        S("fhe_conv_create", C.c_int, [vp, u32p, u32, u32p, u32, C.POINTER(vp)])
        S("fhe_conv_destroy", None, [vp])
        S("fhe_approx_switch_basis", C.c_int, [vp, vp, u32, u32, vp, u32, u32, u32, vp])
        S("fhe_switch_basis_exact", C.c_int, [vp, vp, u32, u32, vp, u32, u32, u32, vp])
        S("fhe_conv_create_custom", C.c_int, [vp, u32p, u32, u32p, u32, u64p, u64p, u64p, C.POINTER(C.c_double), C.POINTER(vp)])
        S("fhe_expand_crt_basis_workspace_bytes", C.c_size_t, [vp, u32])
        S("fhe_expand_crt_basis", C.c_int, [vp, vp, C.c_int, vp, C.c_int, C.c_int, u32, vp, C.c_size_t, vp])
        S("fhe_fast_expand_crt_basis_p_over_q", C.c_int, [vp, vp, vp, vp, u32, vp])
        S("fhe_ks_plan_create", C.c_int, [vp, u32, u32, u32, C.POINTER(vp)])
        S("fhe_ks_plan_destroy", None, [vp])
        S("fhe_ks_plan_alpha", u32, [vp])
        S("fhe_ks_plan_levels_built", u32, [vp])
        S("fhe_ks_key_alloc", C.c_int, [vp, C.POINTER(vp)])
        S("fhe_ks_key_upload", C.c_int, [vp, u64p, u64p, C.POINTER(vp)])
        S("fhe_ks_key_wrap", C.c_int, [vp, vp, vp, C.POINTER(vp)])
        S("fhe_ks_key_destroy", None, [vp])
        S("fhe_ks_key_devptr", vp, [vp, C.c_int])
        S("fhe_ks_key_words", C.c_size_t, [vp])
        S("fhe_keygen_combine", C.c_int, [vp, u32p, u32, u32, u32, vp, vp, vp, u32p, vp, u32p, u64p, u64, vp, vp])
        S("fhe_ks_secret_extend", C.c_int, [vp, vp, vp, vp, C.c_size_t, vp])
        S("fhe_ks_keygen_hybrid", C.c_int, [vp, u32, u32p, u32p, vp, vp, u64, vp, vp, vp, vp])
        S("fhe_ks_keygen_hybrid_blake2", C.c_int, [vp, u32, u32p, u32p, vp, vp, u64, C.c_double, u32p, u64, u64, vp, vp, vp])
        S("fhe_ks_keygen_counters", C.c_int, [vp, u32, u64p, u64p])
        S("fhe_encrypt_pk_combine", C.c_int, [vp, u32p, u32, u32, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp])
        S("fhe_encrypt_sk_combine", C.c_int, [vp, u32p, u32, u32, vp, vp, vp, vp, u64, vp, vp, vp])
        S("fhe_encrypt_chunk", u32, [vp, u32, u32])
        S("fhe_encrypt_workspace_bytes", C.c_size_t, [vp, u32, u32])
        S("fhe_encrypt_pk_blake2", C.c_int,
          [vp, u32p, u32, u32, vp, vp, C.c_int, u64, C.c_double, u32p, u64, u64, vp, C.c_int, vp, vp, C.c_size_t, vp])
        S("fhe_encrypt_sk_blake2", C.c_int, [vp, u32p, u32, u32, vp, u64, C.c_double, u32p, u64, u64, vp, C.c_int, vp, vp])
        S("fhe_encrypt_counters", C.c_int, [vp, u32, u32, C.c_int, u64p, u64p])
        S("fhe_ks_workspace_bytes", C.c_size_t, [vp, u32, u32])
        S("fhe_keyswitch_hybrid", C.c_int, [vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_keyswitch_hybrid_acc", C.c_int, [vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_ckks_eval_mult", C.c_int, [vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_ks_precompute", C.c_int, [vp, vp, u32, u32, vp, C.c_size_t, vp])
        S("fhe_ks_fast_keyswitch", C.c_int, [vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_eval_fast_rotation", C.c_int, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_eval_automorphism", C.c_int, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_ks_ext", C.c_int, [vp, vp, u32, u32, vp, vp])
        S("fhe_ks_fast_keyswitch_ext", C.c_int, [vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_eval_fast_rotation_ext", C.c_int, [vp, vp, vp, vp, u32, C.c_int, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_ks_down", C.c_int, [vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_ckks_bsgs_workspace_bytes", C.c_size_t, [vp, u32, u32, u32, u32])
        S("fhe_ckks_bsgs_transform", C.c_int, [vp, vp, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, C.c_size_t, vp])
        S("fhe_approx_mod_down", C.c_int, [vp, vp, u32, u32, vp, vp, C.c_size_t, vp])
        S("fhe_approx_mod_down_bgv", C.c_int, [vp, vp, u32, u64, u32, vp, vp, C.c_size_t, vp])
        S("fhe_rescale_workspace_bytes", C.c_size_t, [vp, u32, u32])
        S("fhe_rescale", C.c_int, [vp, vp, u32, u32, vp, vp, C.c_size_t, vp])
        S("fhe_rescale_limbs", C.c_int, [vp, vp, u32p, u32, u64p, u64p, u32, vp, vp, C.c_size_t, vp])
        S("fhe_rescale_limbs_pair", C.c_int, [vp, vp, vp, u32p, u32, u64p, u64p, vp, vp, vp, C.c_size_t, vp])
        S("fhe_add_pair", C.c_int, [vp, vp, vp, vp, vp, vp, vp, u32p, u32, vp])
        S("fhe_sub_pair", C.c_int, [vp, vp, vp, vp, vp, vp, vp, u32p, u32, vp])
        S("fhe_mul_const_pair", C.c_int, [vp, vp, vp, vp, vp, u64p, u32p, u32, vp])
        S("fhe_mem_info", C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])
        S("fhe_lincomb", C.c_int, [vp, vp, C.POINTER(vp), u64p, u32, u32p, u32, u32, C.c_int, vp])
        S("fhe_rescale_multi_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_rescale_multi", C.c_int, [vp, vp, u32, u32, u32, u64p, u32, vp, vp, C.c_size_t, vp])
        S("fhe_rescale_multi_limbs", C.c_int, [vp, vp, u32p, u32, u32, u32, u64p, u64p, u64p, u32, vp, vp, C.c_size_t, vp])
        S("fhe_rescale_multi_limbs_pair", C.c_int, [vp, vp, vp, u32p, u32, u32, u32, u64p, u64p, u64p, vp, vp, vp, C.c_size_t, vp])
        S("fhe_rescale_multi_host_tables", C.c_int, [u64p, u32, u64p, u32, u64p, u64p, u64p, u64p, u64p, u64p])
        S("fhe_mod_reduce", C.c_int, [vp, vp, u32, u64, C.c_int, u32, vp, vp, C.c_size_t, vp])
        S("fhe_mod_reduce_limbs", C.c_int, [vp, vp, u32p, u32, u64, u64, u64p, C.c_int, u32, vp, vp, C.c_size_t, vp])
        S("fhe_mod_reduce_limbs_pair", C.c_int, [vp, vp, vp, u32p, u32, u64, u64, u64p, C.c_int, vp, vp, vp, C.c_size_t, vp])
        S("fhe_mod_reduce_multi_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_mod_reduce_multi", C.c_int, [vp, vp, u32, u64, u64, u32p, u32, u32, C.c_int, u32, vp, vp, C.c_size_t, vp])
        S("fhe_mod_reduce_multi_limbs", C.c_int, [vp, vp, u32p, u32, u64, u64, u32p, u32, u32, u64p, u64p, C.c_int, u32, vp, vp, C.c_size_t,
                                                  vp])
        S("fhe_mod_reduce_multi_limbs_pair", C.c_int, [vp, vp, vp, u32p, u32, u64, u64, u32p, u32, u32, u64p, u64p, C.c_int, vp, vp, vp,
                                                       C.c_size_t, vp])
        S("fhe_mod_reduce_multi_host_tables", C.c_int, [u64p, u32, u64p, u32, u64, u64p, u64p, u64p, u64p, u64p, u64p])
        S("fhe_mod_reduce_chain_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_mod_reduce_chain", C.c_int, [vp, vp, u32p, u32, u32, u64, u32, vp, vp, C.c_size_t, vp])
        S("fhe_mod_reduce_to_t", C.c_int, [vp, vp, u32p, u32, u64, u32, vp, vp, C.c_size_t, vp])
        S("fhe_bgv_decrypt_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_bgv_decrypt", C.c_int, [vp, C.POINTER(vp), u32, vp, u32p, u32, u64, u32, vp, vp, C.c_size_t, vp])
        S("fhe_decrypt_core", C.c_int, [vp, C.POINTER(vp), u32, vp, u32p, u32, u32, vp, u64, C.c_int, C.c_int, vp, vp])
        S("fhe_decrypt_chunk", u32, [vp, u32, u32])
        S("fhe_bfv_decrypt_create", C.c_int, [vp, u32p, u32, u64, C.c_int, C.POINTER(vp)])
        S("fhe_bfv_decrypt_destroy", None, [vp])
        S("fhe_bfv_decrypt_workspace_bytes", C.c_size_t, [vp, u32])
        S("fhe_bfv_decrypt_table", C.c_size_t, [vp, C.c_int, u64p, C.c_size_t])
        S("fhe_bfv_decrypt", C.c_int, [vp, C.POINTER(vp), u32, vp, u32, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_decrypt_b", C.c_int, [vp, vp, C.c_int, u32, vp, vp, C.c_size_t, vp])
        S("fhe_bgv_keyswitch_hybrid", C.c_int, [vp, vp, vp, u32, u64, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bgv_keyswitch_hybrid_acc", C.c_int, [vp, vp, vp, u32, u64, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bgv_eval_mult", C.c_int, [vp, vp, vp, vp, vp, vp, u32, u64, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bgv_ks_fast_keyswitch", C.c_int, [vp, vp, vp, u32, u64, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bgv_eval_fast_rotation", C.c_int, [vp, vp, vp, vp, u32, u32, u64, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bgv_eval_automorphism", C.c_int, [vp, vp, vp, vp, u32, u32, u64, u32, vp, vp, vp, C.c_size_t, vp])
        f64p = C.POINTER(C.c_double)
        S("fhe_sr_plan_create", C.c_int, [vp, u32, u32p, u32, u64p, f64p, C.POINTER(vp)])
        S("fhe_sr_plan_destroy", None, [vp])
        S("fhe_scale_and_round", C.c_int, [vp, vp, C.c_int, vp, u32, vp])
        S("fhe_scale_and_round_p_over_q", C.c_int, [vp, vp, u32p, u32, vp, u32, vp])
        S("fhe_scale_and_round_native", C.c_int, [vp, vp, u32p, u32, u64, u64p, u64p, f64p, f64p, u32, vp, vp])
        S("fhe_scale_and_round_behz_decrypt", C.c_int, [vp, vp, u32p, u32, u64, u64p, u64p, u32, vp, vp])
        S("fhe_param_behz_bsk", u32, [u32, u32, u64p, u64, u64p, u64p])
        S("fhe_behz_create", C.c_int, [vp, u32p, u32, u32p, u64, C.POINTER(vp)])
        S("fhe_behz_destroy", None, [vp])
        S("fhe_behz_override_q_to_bsk", C.c_int, [vp, u64p, u64p, u64p, u64p, u64, u64p])
        S("fhe_behz_override_floorq", C.c_int, [vp, u64p, u64p, u64p, u64p])
        S("fhe_behz_override_conv_sk", C.c_int, [vp, u64p, u64p, u64, u64p, u64p])
        S("fhe_behz_workspace_bytes", C.c_size_t, [vp, u32])
        S("fhe_behz_q_to_bsk", C.c_int, [vp, vp, C.c_int, u32, vp, C.c_size_t, vp])
        S("fhe_behz_floorq", C.c_int, [vp, vp, u32, vp])
        S("fhe_behz_conv_sk", C.c_int, [vp, vp, vp, u32, vp])
        S("fhe_bfv_eval_mult_behz_workspace_bytes", C.c_size_t, [vp, u32])
        S("fhe_bfv_eval_mult_behz", C.c_int, [vp] * 8 + [C.c_int, u32, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_mult_relin_workspace_bytes", C.c_size_t, [vp, vp, u32])
        S("fhe_param_hps_r", u32, [u32, u32, u64p, C.c_int, u64p, u64p])
        S("fhe_hps_create", C.c_int, [vp, u32p, u32, u32p, u32, u64, C.c_int, C.POINTER(vp)])
        S("fhe_hps_destroy", None, [vp])
        S("fhe_hps_table", C.c_size_t, [vp, C.c_int, u32, u64p, C.c_size_t])
        S("fhe_bfv_eval_mult_hps_workspace_bytes", C.c_size_t, [vp, u32, u32])
        S("fhe_bfv_eval_mult_hps", C.c_int, [vp] * 8 + [u32, C.c_int, u32, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_mult_relin_behz", C.c_int, [vp] * 9 + [u32, vp, C.c_size_t, vp])
        S("fhe_bv_key_upload", C.c_int, [vp, u32, u32, u64p, u64p, C.POINTER(vp)])
        S("fhe_bv_key_wrap", C.c_int, [vp, u32, u32, vp, vp, C.POINTER(vp)])
        S("fhe_bv_key_destroy", None, [vp])
        S("fhe_bv_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_bv_precompute", C.c_int, [vp, vp, C.c_int, u32, u32, u32, vp, C.c_size_t, vp])
        S("fhe_bv_fast_keyswitch", C.c_int, [vp, u32, u32, vp, vp, C.c_int, vp, C.c_size_t, vp])
        S("fhe_keyswitch_bv", C.c_int, [vp, vp, u32, u32, vp, vp, C.c_int, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_mult_relin_hps_bv_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_bfv_eval_mult_relin_hps_bv", C.c_int, [vp] * 8 + [u32, u32, vp, C.c_size_t, vp])
        S("fhe_bv_eval_fast_rotation", C.c_int, [vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bv_eval_automorphism", C.c_int, [vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_bv_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_bfv_fast_rotation_precompute_bv", C.c_int, [vp, vp, u32, u32, u32, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_fast_rotation_bv", C.c_int, [vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_automorphism_bv", C.c_int, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_relinearize_bv", C.c_int, [vp] * 5 + [C.c_int, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_mult_relin_hps_bv_leveled_workspace_bytes", C.c_size_t, [vp, u32, u32, u32, u32])
        S("fhe_bfv_eval_mult_relin_hps_bv_leveled", C.c_int, [vp] * 8 + [u32, u32, u32, vp, C.c_size_t, vp])
        S("fhe_bv_keygen_factors", u32, [vp, u32, u32, u64p])
        S("fhe_bv_keygen", C.c_int, [vp, u32, u32, u32, u32p, u32p, vp, vp, u64, vp, vp, vp, vp])
        S("fhe_bv_keygen_blake2", C.c_int, [vp, u32, u32, u32, u32p, u32p, vp, vp, u64, C.c_double, u32p, u64, u64, vp, vp, vp])
        S("fhe_bv_keygen_counters", C.c_int, [vp, u32, u32, u32, C.c_int, u64p, u64p])
        S("fhe_bv_keygen_pk", C.c_int, [vp, u32, u32, u32, vp, vp, C.c_int, vp, u64, vp, vp, vp, vp, vp, vp])
        S("fhe_bv_keygen_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_bv_keygen_pk_blake2", C.c_int,
          [vp, u32, u32, u32, vp, vp, C.c_int, vp, C.c_int, u64, C.c_double, u32p, u64, u64, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_hybrid_create", C.c_int, [vp, vp, C.POINTER(vp)])
        S("fhe_bfv_hybrid_destroy", None, [vp])
        S("fhe_bfv_hybrid_workspace_bytes", C.c_size_t, [vp, u32, u32])
        S("fhe_bfv_fast_rotation_precompute_hybrid", C.c_int, [vp, vp, u32, u32, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_fast_rotation_hybrid", C.c_int, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_automorphism_hybrid", C.c_int, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_relinearize_hybrid", C.c_int, [vp] * 5 + [C.c_int, u32, u32, vp, vp, vp, C.c_size_t, vp])
        S("fhe_bfv_eval_mult_relin_hps_hybrid_workspace_bytes", C.c_size_t, [vp, u32, u32, u32])
        S("fhe_bfv_eval_mult_relin_hps_hybrid", C.c_int, [vp] * 8 + [u32, u32, u32, vp, C.c_size_t, vp])
        S("fhe_param_first_prime", u64, [u32, u64])
        S("fhe_param_last_prime", u64, [u32, u64])
        S("fhe_param_next_prime", u64, [u64, u64])
        S("fhe_param_previous_prime", u64, [u64, u64])
        S("fhe_param_root_of_unity", u64, [u64, u64])
        S("fhe_param_dcrt_chain", C.c_int, [u32, u32, u32, u64p, u64p])
        S("fhe_param_select_p", u32, [u32, u32, u64p, u32, u32, u64p, u64p])
        S("fhe_param_find_automorphism_index_2n_complex", u32, [C.c_int32, u32])
        S("fhe_launch_stats", C.c_size_t, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64)])
        S("fhe_time_ntt", C.c_int, [vp, vp, u32p, u32, u32, C.c_int, C.c_int, vp, C.POINTER(C.c_float)])

    def check(self, status):
        if status != 0:
            raise FheError(f"fhe status {status}: {self.L.fhe_last_error().decode()}")

    def launch_count(self, kernel):
        """launches of `kernel` (name without template arguments) since the library was loaded (fhe_launch_stats)"""
        buf = C.create_string_buffer(1 << 16)
        self.L.fhe_launch_stats(buf, len(buf), None)
        for line in buf.value.decode().splitlines():
            k, n = line.rsplit(" ", 1)
            if k.split("::")[-1] == kernel:
                return int(n)
        return 0

    def handover_counts(self):
        """launches of the hand-over instances since the library was loaded: (inverse row pass, inverse column pass)"""
        return self.launch_count("ntt_row8_batched_kernel<HAND>"), self.launch_count("ntt_static_kernel<HAND>")

    def blake2xb_stream(self, key, counter0, n_blocks):
        """uint32[n_blocks][1024]: the 4 KiB blocks blake2xb(in = counter0 + k, key) of Blake2Engine (fhe_blake2xb_stream)"""
        if getattr(self, "_tiny", None) is None:
            # the smallest context the library builds (N = 16, q = 97 = 1 mod 32, 19 a primitive 32nd root of unity): it only names the device
            self._tiny = Context(self, 4, [97], [19])
        return self._tiny.blake2xb_stream(key, counter0, n_blocks)

    def version(self):
        return self.L.fhe_version().decode()

    def device_count(self):
        return self.L.fhe_device_count()

    # ---- host-side parameter helpers (ILDCRTParams chain, HYBRID auxiliary basis) ----
    def dcrt_chain(self, logN, n_limbs, bits):
        q = np.zeros(n_limbs, np.uint64)
        psi = np.zeros(n_limbs, np.uint64)
        self.check(self.L.fhe_param_dcrt_chain(2 << logN, n_limbs, bits, q.ctypes.data_as(u64p), psi.ctypes.data_as(u64p)))
        return q, psi

    def ckks_like_chain(self, logN, sizeQ, first_bits=60, scale_bits=59):
        """first modulus of first_bits, then sizeQ-1 descending primes of scale_bits (FIXEDMANUAL-like shape)"""
        M = 2 << logN
        q = [self.L.fhe_param_last_prime(first_bits, M)]
        cur = self.L.fhe_param_last_prime(scale_bits, M)
        while len(q) < sizeQ:
            if cur not in q:
                q.append(cur)
            cur = self.L.fhe_param_previous_prime(cur, M)
        q = np.array(q, np.uint64)
        psi = np.array([self.L.fhe_param_root_of_unity(M, int(v)) for v in q], np.uint64)
        return q, psi

    def behz_bsk(self, logN, q, t):
        q = np.ascontiguousarray(q, dtype=np.uint64)
        bsk = np.zeros(len(q) + 1, np.uint64)
        psi = np.zeros(len(q) + 1, np.uint64)
        n = self.L.fhe_param_behz_bsk(logN, len(q), q.ctypes.data_as(u64p), t, bsk.ctypes.data_as(u64p), psi.ctypes.data_as(u64p))
        if n == 0:
            raise FheError("fhe_param_behz_bsk failed")
        return bsk, psi

    def hps_r(self, logN, q, technique):
        """the auxiliary basis R of BFV's HPS family (bfvrns-cryptoparameters.cpp:75, 126-139): (moduli, roots)"""
        q = np.ascontiguousarray(q, dtype=np.uint64)
        r = np.zeros(len(q) + 1, np.uint64)
        psi = np.zeros(len(q) + 1, np.uint64)
        n = self.L.fhe_param_hps_r(logN, len(q), q.ctypes.data_as(u64p), technique, r.ctypes.data_as(u64p), psi.ctypes.data_as(u64p))
        if n == 0:
            raise FheError("fhe_param_hps_r failed")
        return r[:n].copy(), psi[:n].copy()

    def find_automorphism_index(self, index, m):
        """FindAutomorphismIndex2nComplex (nbtheory2.cpp:243-262)"""
        k = self.L.fhe_param_find_automorphism_index_2n_complex(index, m)
        if k == 0:
            raise FheError("m should be a power of two.")
        return k

    def select_p(self, logN, q, numPartQ, aux_bits=60):
        q = np.ascontiguousarray(q, dtype=np.uint64)
        p = np.zeros(64, np.uint64)
        psi = np.zeros(64, np.uint64)
        n = self.L.fhe_param_select_p(logN, len(q), q.ctypes.data_as(u64p), numPartQ, aux_bits, p.ctypes.data_as(u64p),
                                      psi.ctypes.data_as(u64p))
        if n == 0:
            raise FheError("fhe_param_select_p failed")
        return p[:n].copy(), psi[:n].copy()


class Context:
    """Ring dimension N = 2^logN + modulus tower (q_i, psi_i) with device-resident twiddle tables."""

    def __init__(self, lib, logN, q, psi, device=0):
        self.lib, self.logN, self.N = lib, logN, 1 << logN
        self.q = np.ascontiguousarray(np.asarray(q, dtype=np.uint64))
        self.psi = np.ascontiguousarray(np.asarray(psi, dtype=np.uint64))
        self.L = len(self.q)
        h = vp()
        lib.check(lib.L.fhe_ctx_create(logN, self.L, self.q.ctypes.data_as(u64p), self.psi.ctypes.data_as(u64p),
                                       device, C.byref(h)))
        self.h = h
        self._allocs = {}  # pointer value -> handle

    def close(self):
        if self.h:
            for p in self._allocs.values():
                self.lib.L.fhe_free(self.h, p)
            self._allocs = {}
            self.lib.L.fhe_ctx_destroy(self.h)
            self.h = None

    # ---- raw device memory ----
    def malloc(self, nbytes):
        p = vp()
        self.lib.check(self.lib.L.fhe_malloc(self.h, nbytes, C.byref(p)))
        self._allocs[p.value] = p
        return p

    def free(self, p):
        if self._allocs.pop(p.value, None) is not None:
            self.lib.check(self.lib.L.fhe_free(self.h, p))

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        p = self.malloc(arr.nbytes)
        self.lib.check(self.lib.L.fhe_memcpy_h2d(self.h, p, arr.ctypes.data_as(vp), arr.nbytes, stream))
        self.sync(stream)
        return p

    def download(self, p, shape, stream=None):
        out = np.empty(shape, dtype=np.uint64)
        self.lib.check(self.lib.L.fhe_memcpy_d2h(self.h, out.ctypes.data_as(vp), p, out.nbytes, stream))
        self.sync(stream)
        return out

    def sync(self, stream=None):
        self.lib.check(self.lib.L.fhe_stream_sync(self.h, stream))

    def checksum(self, tower, stream=None):
        """uint64[batch * limbs][2] = {sum, position-weighted sum} mod 2^64 of every limb-row of the tower (fhe_checksum)"""
        rows = tower.batch * tower.n_limbs
        d = self.malloc(rows * 16)
        try:
            self.lib.check(self.lib.L.fhe_checksum(self.h, tower.ptr, rows, d, stream))
            return self.download(d, (rows, 2), stream)
        finally:
            self.free(d)

    def tower(self, host, limb_idx=None, fmt=EVALUATION):
        """host: uint64 [batch][nLimbs][N] (or [nLimbs][N])"""
        host = np.asarray(host, dtype=np.uint64)
        if host.ndim == 2:
            host = host[None]
        return Tower(self, self.upload(host), host.shape[0], host.shape[1], limb_idx, fmt, owned=True)

    def empty(self, batch, n_limbs, limb_idx=None, fmt=EVALUATION):
        return Tower(self, self.malloc(batch * n_limbs * self.N * 8), batch, n_limbs, limb_idx, fmt, owned=True)

    # ---- sampled towers (the sampling constructors of DCRTPolyImpl, dcrtpoly-impl.h:126-205, on the device: fhe_sample_*) ----
    def sample(self, kind, batch, n_limbs, seed=0, stream_id=0, limb_idx=None, sigma=3.19, stream=None, generator="philox", key=None,
               counter0=0):
        """kind: "uniform" (DugType), "gaussian" (DggType, standard deviation sigma) or "ternary" (TugType); COEFFICIENT format.
        generator "philox": Philox4x32-10 keyed by `seed`, sub-stream `stream_id` (fhe_sample_*; a statistical generator);
        generator "blake2": the reference's blake2xb counter mode keyed by `key` (64 bytes or 16 uint32 words) from block `counter0`
        (fhe_sample_*_blake2)"""
        t = self.empty(batch, n_limbs, limb_idx, COEFFICIENT)
        L = self.lib.L
        if generator == "blake2":
            k = _key_words(key)
            kp = k.ctypes.data_as(u32p)
            if kind == "uniform":
                self.lib.check(L.fhe_sample_uniform_blake2(self.h, t.ptr, t._li(), n_limbs, batch, kp, counter0, stream))
            elif kind == "gaussian":
                self.lib.check(L.fhe_sample_gaussian_blake2(self.h, t.ptr, t._li(), n_limbs, batch, sigma, kp, counter0, stream))
            elif kind == "ternary":
                self.lib.check(L.fhe_sample_ternary_blake2(self.h, t.ptr, t._li(), n_limbs, batch, kp, counter0, stream))
            else:
                raise ValueError(kind)
            return t
        if generator != "philox":
            raise ValueError(generator)
        if kind == "uniform":
            self.lib.check(L.fhe_sample_uniform(self.h, t.ptr, t._li(), n_limbs, batch, seed, stream_id, stream))
        elif kind == "gaussian":
            self.lib.check(L.fhe_sample_gaussian(self.h, t.ptr, t._li(), n_limbs, batch, sigma, seed, stream_id, stream))
        elif kind == "ternary":
            self.lib.check(L.fhe_sample_ternary(self.h, t.ptr, t._li(), n_limbs, batch, seed, stream_id, stream))
        else:
            raise ValueError(kind)
        return t


    def blake2xb_stream(self, key, counter0, n_blocks, stream=None):
        """uint32[n_blocks][1024]: word i of row k is word i of blake2xb(4096 bytes, in = counter0 + k, key) (fhe_blake2xb_stream)"""
        k = _key_words(key)
        d = self.malloc(max(n_blocks, 1) * 4096)
        try:
            self.lib.check(self.lib.L.fhe_blake2xb_stream(self.h, d, n_blocks, k.ctypes.data_as(u32p), counter0, stream))
            return self.download(d, (n_blocks, 512), stream).view(np.uint32)
        finally:
            self.free(d)


def _key_words(key):
    """the 512-bit blake2xb key as 16 little-endian uint32 words (Blake2Engine's seed array)"""
    if key is None:
        raise ValueError("generator='blake2' needs a 64-byte key")
    if isinstance(key, (bytes, bytearray)):
        if len(key) != 64:
            raise ValueError("a blake2xb key is 64 bytes")
        return np.frombuffer(bytes(key), dtype="<u4").astype(np.uint32)
    k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32))
    if k.shape != (16,):
        raise ValueError("a blake2xb key is 16 uint32 words")
    return k


class Tower:
    """A batch of device-resident RNS towers: the DCRTPoly data model, uint64[batch][nLimbs][N]."""

    def __init__(self, ctx, ptr, batch, n_limbs, limb_idx=None, fmt=EVALUATION, owned=False):
        self.ctx, self.ptr, self.batch, self.n_limbs, self.fmt = ctx, ptr, batch, n_limbs, fmt
        self._owned = owned  # allocated by Context.tower()/empty(): freed with the object
        self.limb_idx = None if limb_idx is None else np.ascontiguousarray(np.asarray(limb_idx, dtype=np.uint32))

    def _li(self):
        return None if self.limb_idx is None else self.limb_idx.ctypes.data_as(u32p)

    def to_host(self):
        return self.ctx.download(self.ptr, (self.batch, self.n_limbs, self.ctx.N))

    def like(self):
        return self.ctx.empty(self.batch, self.n_limbs, self.limb_idx, self.fmt)

    def free(self):
        """release the device buffer now (a Tower that is simply dropped is released by the garbage collector)"""
        if self.ptr is not None and self.ctx.h:
            self.ctx.free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            if getattr(self, "_owned", False):
                self.free()
        except Exception:
            pass

    def MultAccEqNoCheck(self, v, consts, stream=None):  # poly.h:323 / mubintvecnat.cpp:132-142, per limb
        consts = np.ascontiguousarray(np.asarray(consts, dtype=np.uint64))
        self.ctx.lib.check(self.ctx.lib.L.fhe_mult_acc(self.ctx.h, self.ptr, v.ptr, consts.ctypes.data_as(u64p), self._li(),
                                                      self.n_limbs, self.batch, stream))
        return self

    # DCRTPolyImpl::SwitchFormat (dcrtpoly-impl.h:1932-1940)
    def SwitchFormat(self, stream=None):
        L, c = self.ctx.lib, self.ctx
        f = L.L.fhe_ntt_inv if self.fmt == EVALUATION else L.L.fhe_ntt_fwd
        L.check(f(c.h, self.ptr, self._li(), self.n_limbs, self.batch, stream))
        self.fmt = COEFFICIENT if self.fmt == EVALUATION else EVALUATION
        return self

    def SetFormat(self, fmt, stream=None):  # ilelement.h:447-450
        if fmt != self.fmt:
            self.SwitchFormat(stream)
        return self

    # DCRTPolyImpl::CRTDecompose(baseBits) (dcrtpoly-impl.h:230-285): the towers of KeySwitchBV's digit decomposition, EVALUATION format,
    # as ONE batch [towers][nLimbs][N] (batch must be 1; None when the digit size is outside the device path)
    def CRTDecompose(self, base_bits, stream=None):
        assert self.batch == 1
        L, c = self.ctx.lib, self.ctx
        towers = L.L.fhe_crt_decompose_towers(c.h, self._li(), self.n_limbs, base_bits)
        if towers == 0:
            return None
        src = self
        if self.fmt == EVALUATION:  # (:231-233: the coefficient copy)
            src = c.empty(1, self.n_limbs, self.limb_idx, COEFFICIENT)
            L.check(L.L.fhe_ntt_inv_oop(c.h, self.ptr, src.ptr, self._li(), self.n_limbs, 1, stream))
        out = c.empty(towers, self.n_limbs, self.limb_idx, EVALUATION)
        L.check(L.L.fhe_crt_decompose(c.h, src.ptr, self._li(), self.n_limbs, base_bits, out.ptr, stream))
        return out

    def _bin(self, fn, other, stream):
        out = self.like()
        self.ctx.lib.check(fn(self.ctx.h, out.ptr, self.ptr, other.ptr, self._li(), self.n_limbs, self.batch, stream))
        return out

    def Plus(self, other, stream=None):  # dcrtpoly.h:153-162
        return self._bin(self.ctx.lib.L.fhe_add, other, stream)

    def Minus(self, other, stream=None):  # dcrtpoly-impl.h:362-371
        return self._bin(self.ctx.lib.L.fhe_sub, other, stream)

    def Times(self, other, stream=None):  # dcrtpoly.h:174-189
        if isinstance(other, Tower):
            return self._bin(self.ctx.lib.L.fhe_mul, other, stream)
        consts = np.ascontiguousarray(np.asarray(other, dtype=np.uint64))  # Times(vector<NativeInteger>) :582-601
        out = self.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_mul_const(self.ctx.h, out.ptr, self.ptr, consts.ctypes.data_as(u64p),
                                                       self._li(), self.n_limbs, self.batch, stream))
        return out

    def PolyMul(self, other, stream=None):
        """negacyclic product of two COEFFICIENT towers (fhe_poly_mul): INTT(NTT(a) o NTT(b)) per limb"""
        L = self.ctx.lib.L
        out = self.like()
        wsb = L.fhe_poly_mul_workspace_bytes(self.ctx.h, self.n_limbs, self.batch)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_poly_mul(self.ctx.h, self.ptr, other.ptr, out.ptr, self._li(), self.n_limbs, self.batch, ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return out

    def Negate(self, stream=None):  # dcrtpoly-impl.h:347-354
        out = self.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_neg(self.ctx.h, out.ptr, self.ptr, self._li(), self.n_limbs, self.batch,
                                                  stream))
        return out

    def AutomorphismTransform(self, k, stream=None):  # dcrtpoly-impl.h:314-333
        out = self.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_automorph(self.ctx.h, out.ptr, self.ptr, k,
                                                        1 if self.fmt == EVALUATION else 0, self._li(), self.n_limbs,
                                                        self.batch, stream))
        return out


class Conv:
    """CRT basis conversion plan (ApproxSwitchCRTBasis / SwitchCRTBasis)."""

    def __init__(self, ctx, src_idx, dst_idx, hat_inv=None, hat_mod=None, alpha_mod=None, q_inv=None):
        """default: the plain CRT tables of (src basis, dst basis); with hat_inv[nSrc] / hat_mod[nSrc][nDst]
        (+ alpha_mod[nSrc+1][nDst], q_inv[nSrc] for the exact variant) the caller's tables (fhe_conv_create_custom)"""
        self.ctx = ctx
        self.src = np.ascontiguousarray(np.asarray(src_idx, dtype=np.uint32))
        self.dst = np.ascontiguousarray(np.asarray(dst_idx, dtype=np.uint32))
        h = vp()
        if hat_inv is None:
            ctx.lib.check(ctx.lib.L.fhe_conv_create(ctx.h, self.src.ctypes.data_as(u32p), len(self.src),
                                                    self.dst.ctypes.data_as(u32p), len(self.dst), C.byref(h)))
        else:
            hi = np.ascontiguousarray(hat_inv, dtype=np.uint64)
            hm = np.ascontiguousarray(hat_mod, dtype=np.uint64)
            assert hm.shape == (len(self.src), len(self.dst))
            al = qi = None
            if alpha_mod is not None:
                al_a = np.ascontiguousarray(alpha_mod, dtype=np.uint64)
                qi_a = np.ascontiguousarray(q_inv, dtype=np.float64)
                al, qi = al_a.ctypes.data_as(u64p), qi_a.ctypes.data_as(C.POINTER(C.c_double))
            ctx.lib.check(ctx.lib.L.fhe_conv_create_custom(ctx.h, self.src.ctypes.data_as(u32p), len(self.src),
                                                           self.dst.ctypes.data_as(u32p), len(self.dst),
                                                           hi.ctypes.data_as(u64p), hm.ctypes.data_as(u64p), al, qi,
                                                           C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.L.fhe_conv_destroy(self.h)
            self.h = None

    def run(self, tin, exact=False, stream=None):
        """tin: Tower [batch][nSrc][N] COEFFICIENT -> Tower [batch][nDst][N] COEFFICIENT"""
        out = self.ctx.empty(tin.batch, len(self.dst), self.dst, COEFFICIENT)
        f = self.ctx.lib.L.fhe_switch_basis_exact if exact else self.ctx.lib.L.fhe_approx_switch_basis
        self.ctx.lib.check(f(self.h, tin.ptr, tin.n_limbs, 0, out.ptr, len(self.dst), 0, tin.batch, stream))
        return out

    def ExpandCRTBasis(self, tin, result_format, reverse=False, stream=None):
        """DCRTPoly::ExpandCRTBasis[ReverseOrder] (dcrtpoly-impl.h:1088-1148): tower over the source basis -> Q u P"""
        idx = np.concatenate([self.dst, self.src]) if reverse else np.concatenate([self.src, self.dst])
        out = self.ctx.empty(tin.batch, len(idx), idx, result_format)
        L = self.ctx.lib.L
        wsb = L.fhe_expand_crt_basis_workspace_bytes(self.h, tin.batch)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_expand_crt_basis(self.h, tin.ptr, 1 if tin.fmt == EVALUATION else 0, out.ptr,
                                                      1 if result_format == EVALUATION else 0, 1 if reverse else 0,
                                                      tin.batch, ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return out

    def ApproxModUp(self, tin, stream=None):
        """DCRTPoly::ApproxModUp (dcrtpoly-impl.h:935-963): tower over the source basis (either format) -> Q u P, EVALUATION"""
        idx = np.concatenate([self.src, self.dst])
        out = self.ctx.empty(tin.batch, len(idx), idx, EVALUATION)
        L = self.ctx.lib.L
        wsb = L.fhe_expand_crt_basis_workspace_bytes(self.h, tin.batch)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_mod_up(self.h, tin.ptr, 1 if tin.fmt == EVALUATION else 0, out.ptr, tin.batch, ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return out

    def FastExpandCRTBasisPloverQ(self, to_ql, tin, stream=None):
        """self = custom-table plan Q -> Pl, to_ql = plan Pl -> Ql (dcrtpoly-impl.h:1151-1164); COEFFICIENT towers"""
        idx = np.concatenate([to_ql.dst, self.dst])
        out = self.ctx.empty(tin.batch, len(idx), idx, COEFFICIENT)
        self.ctx.lib.check(self.ctx.lib.L.fhe_fast_expand_crt_basis_p_over_q(self.h, to_ql.h, tin.ptr, out.ptr, tin.batch, stream))
        return out


class KeySwitchPlan:
    """HYBRID key switching for a context whose limbs are Q (sizeQ) followed by P (sizeP)."""

    def __init__(self, ctx, sizeQ, sizeP, numPartQ):
        self.ctx, self.sizeQ, self.sizeP, self.numPartQ = ctx, sizeQ, sizeP, numPartQ
        h = vp()
        ctx.lib.check(ctx.lib.L.fhe_ks_plan_create(ctx.h, sizeQ, sizeP, numPartQ, C.byref(h)))
        self.h = h
        self.key = None
        self._ws = None
        self._ws_bytes = 0

    def close(self):
        if self.key:
            self.ctx.lib.L.fhe_ks_key_destroy(self.key)
            self.key = None
        if self.h:
            self.ctx.lib.L.fhe_ks_plan_destroy(self.h)
            self.h = None

    def upload_key(self, keyB, keyA):
        keyB = np.ascontiguousarray(keyB, dtype=np.uint64)
        keyA = np.ascontiguousarray(keyA, dtype=np.uint64)
        k = vp()
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_key_upload(self.h, keyB.ctypes.data_as(u64p),
                                                            keyA.ctypes.data_as(u64p), C.byref(k)))
        self.key = k

    def wrap_key(self, dev_b, dev_a):
        """adopt device-resident key vectors (e.g. torch tensors filled by an RCCL broadcast)"""
        k = vp()
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_key_wrap(self.h, vp(dev_b), vp(dev_a), C.byref(k)))
        self.key = k

    def key_words(self):
        N = self.ctx.N
        return self.numPartQ * (self.sizeQ + self.sizeP) * N

    # ---- key generation on the device (KeySwitchHYBRID::KeySwitchGenInternal, keyswitch-hybrid.cpp:51-130) ----
    def extend_secret(self, s, stream=None):
        """the sNewExt block (:59-83): s [1][sizeQ][N] EVALUATION -> [1][sizeQ+sizeP][N] EVALUATION (fhe_ks_secret_extend)"""
        assert s.batch == 1 and s.n_limbs == self.sizeQ and s.fmt == EVALUATION
        out = self.ctx.empty(1, self.sizeQ + self.sizeP)
        ws = self.ctx.malloc(self.ctx.N * 8)
        try:
            self.ctx.lib.check(self.ctx.lib.L.fhe_ks_secret_extend(self.h, s.ptr, out.ptr, ws, self.ctx.N * 8, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return out

    def keygen_counters(self, n_keys):
        """(blake2 counters keygen_blake2 consumes from counter_a, from counter_e) (fhe_ks_keygen_counters)"""
        na, ne = u64(), u64()
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_keygen_counters(self.h, n_keys, C.byref(na), C.byref(ne)))
        return na.value, ne.value

    def _wrap_keys(self, b, a, n_keys, rotations):
        words = self.key_words()
        keys = []
        for i in range(n_keys):
            k = vp()
            self.ctx.lib.check(self.ctx.lib.L.fhe_ks_key_wrap(self.h, vp(b.ptr.value + 8 * words * i), vp(a.ptr.value + 8 * words * i),
                                                              C.byref(k)))
            keys.append(k)
        return keys if rotations is None else dict(zip(rotations, keys))

    def _keygen_indices(self, n_keys, k_new, k_old, rotations):
        if rotations is not None:
            assert k_new is None and k_old is None and len(rotations) == n_keys
            k_new, k_old = rotation_key_indices(self.ctx.lib, rotations, self.ctx.N)
        kn, knp = _np_u32(k_new)
        ko, kop = _np_u32(k_old)
        assert (kn is None or len(kn) == n_keys) and (ko is None or len(ko) == n_keys)
        return (kn, ko), knp, kop

    def keygen(self, s_new_ext, s_old, a, e, k_new=None, k_old=None, ns=1, rotations=None, in_place=False, stream=None):
        """fhe_ks_keygen_hybrid with the caller's a and e, Towers [nKeys * numPartQ][sizeQ+sizeP][N] in EVALUATION format; s_new_ext from
        extend_secret, s_old [1][sizeQ][N].  k_new / k_old: automorphism indices per key (None = 1), or rotations = CKKS rotation indices
        (rotation_key_indices).  in_place: b overwrites e.  Returns (b, a, keys): the two slabs and the wrapped key handles, a dict by
        rotation index when rotations were given; the slabs own the memory the handles point into."""
        n_keys, rem = divmod(a.batch, self.numPartQ)
        assert rem == 0 and e.batch == a.batch and a.n_limbs == e.n_limbs == self.sizeQ + self.sizeP
        keep, knp, kop = self._keygen_indices(n_keys, k_new, k_old, rotations)
        b = e if in_place else e.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_keygen_hybrid(self.h, n_keys, knp, kop, s_new_ext.ptr, s_old.ptr, ns, a.ptr, e.ptr, b.ptr,
                                                               stream))
        return b, a, self._wrap_keys(b, a, n_keys, rotations)

    def keygen_blake2(self, s_new_ext, s_old, n_keys, key, counter_a, counter_e, k_new=None, k_old=None, ns=1, sigma=3.19, rotations=None,
                      stream=None):
        """fhe_ks_keygen_hybrid_blake2: a = the uniform blake2 sampler's words from counter_a, e = the Gaussian sampler's from counter_e
        (transformed and combined in the buffer that ends up holding b).  Returns (b, a, keys) as keygen does."""
        keep, knp, kop = self._keygen_indices(n_keys, k_new, k_old, rotations)
        b = self.ctx.empty(n_keys * self.numPartQ, self.sizeQ + self.sizeP)
        a = self.ctx.empty(n_keys * self.numPartQ, self.sizeQ + self.sizeP)
        kw = _key_words(key)
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_keygen_hybrid_blake2(self.h, n_keys, knp, kop, s_new_ext.ptr, s_old.ptr, ns, sigma,
                                                                      kw.ctypes.data_as(u32p), counter_a, counter_e, b.ptr, a.ptr, stream))
        return b, a, self._wrap_keys(b, a, n_keys, rotations)

    def destroy_keys(self, keys):
        """release key handles made by keygen / keygen_blake2 / make_key (the slabs of wrapped keys stay with their Towers)"""
        for k in (keys.values() if isinstance(keys, dict) else keys):
            self.ctx.lib.L.fhe_ks_key_destroy(k)

    def workspace(self, sizeQl, batch):
        need = self.ctx.lib.L.fhe_ks_workspace_bytes(self.h, sizeQl, batch)
        if need > self._ws_bytes:
            if self._ws is not None:
                self.ctx.free(self._ws)
            self._ws = self.ctx.malloc(need)
            self._ws_bytes = need
        return self._ws, self._ws_bytes

    # t = 0: CKKS / BFV; t >= 2: the BGV form with the plaintext modulus t (the fhe_bgv_* twin of the entry point)
    def KeySwitchCore(self, c, stream=None, t=0):  # keyswitch-hybrid.cpp:308-312
        ws, wsb = self.workspace(c.n_limbs, c.batch)
        o0, o1 = c.like(), c.like()
        L = self.ctx.lib.L
        if t:
            self.ctx.lib.check(L.fhe_bgv_keyswitch_hybrid(self.h, self.key, c.ptr, c.n_limbs, t, c.batch, o0.ptr, o1.ptr, ws, wsb, stream))
        else:
            self.ctx.lib.check(L.fhe_keyswitch_hybrid(self.h, self.key, c.ptr, c.n_limbs, c.batch, o0.ptr, o1.ptr, ws, wsb, stream))
        return o0, o1

    def KeySwitchCoreAcc(self, c, acc0, acc1, stream=None, t=0):  # base-leveledshe.cpp:207-211: acc += KeySwitchCore(c), in place
        ws, wsb = self.workspace(c.n_limbs, c.batch)
        L = self.ctx.lib.L
        if t:
            self.ctx.lib.check(L.fhe_bgv_keyswitch_hybrid_acc(self.h, self.key, c.ptr, c.n_limbs, t, c.batch, acc0.ptr, acc1.ptr, ws, wsb,
                                                              stream))
        else:
            self.ctx.lib.check(L.fhe_keyswitch_hybrid_acc(self.h, self.key, c.ptr, c.n_limbs, c.batch, acc0.ptr, acc1.ptr, ws, wsb, stream))

    def EvalMult(self, a0, a1, b0, b1, stream=None, t=0):  # base-leveledshe.cpp:201-214
        ws, wsb = self.workspace(a0.n_limbs, a0.batch)
        c0, c1 = a0.like(), a0.like()
        L = self.ctx.lib.L
        if t:
            self.ctx.lib.check(L.fhe_bgv_eval_mult(self.h, self.key, a0.ptr, a1.ptr, b0.ptr, b1.ptr, a0.n_limbs, t, a0.batch, c0.ptr,
                                                   c1.ptr, ws, wsb, stream))
        else:
            self.ctx.lib.check(L.fhe_ckks_eval_mult(self.h, self.key, a0.ptr, a1.ptr, b0.ptr, b1.ptr, a0.n_limbs, a0.batch, c0.ptr,
                                                    c1.ptr, ws, wsb, stream))
        return c0, c1

    def FastKeySwitch(self, key, c1, stream=None, t=0):  # keyswitch-hybrid.cpp:381-400 on the digits EvalFastRotationPrecompute(c1) left
        ws, wsb = self.workspace(c1.n_limbs, c1.batch)
        o0, o1 = c1.like(), c1.like()
        L = self.ctx.lib.L
        if t:
            self.ctx.lib.check(L.fhe_bgv_ks_fast_keyswitch(self.h, key, c1.ptr, c1.n_limbs, t, c1.batch, o0.ptr, o1.ptr, ws, wsb, stream))
        else:
            self.ctx.lib.check(L.fhe_ks_fast_keyswitch(self.h, key, c1.ptr, c1.n_limbs, c1.batch, o0.ptr, o1.ptr, ws, wsb, stream))
        return o0, o1

    def make_key(self, keyB, keyA):
        """upload an additional evaluation key (e.g. a rotation key); returns the handle"""
        keyB = np.ascontiguousarray(keyB, dtype=np.uint64)
        keyA = np.ascontiguousarray(keyA, dtype=np.uint64)
        k = vp()
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_key_upload(self.h, keyB.ctypes.data_as(u64p), keyA.ctypes.data_as(u64p),
                                                            C.byref(k)))
        return k

    def EvalFastRotationPrecompute(self, c1, stream=None):  # base-leveledshe.cpp:425-430
        ws, wsb = self.workspace(c1.n_limbs, c1.batch)
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_precompute(self.h, c1.ptr, c1.n_limbs, c1.batch, ws, wsb, stream))

    def EvalFastRotation(self, key, c0, c1, k, stream=None, t=0):  # base-leveledshe.cpp:432-463 (digits already in ws)
        ws, wsb = self.workspace(c0.n_limbs, c0.batch)
        o0, o1 = c0.like(), c0.like()
        L = self.ctx.lib.L
        if t:
            self.ctx.lib.check(L.fhe_bgv_eval_fast_rotation(self.h, key, c0.ptr, c1.ptr, k, c0.n_limbs, t, c0.batch, o0.ptr, o1.ptr, ws,
                                                            wsb, stream))
        else:
            self.ctx.lib.check(L.fhe_eval_fast_rotation(self.h, key, c0.ptr, c1.ptr, k, c0.n_limbs, c0.batch, o0.ptr, o1.ptr, ws, wsb,
                                                        stream))
        return o0, o1

    def ext_limbs(self, sizeQl):
        """context limbs of the extended basis Q_l u P"""
        return np.concatenate([np.arange(sizeQl), np.arange(self.sizeQ, self.sizeQ + self.sizeP)]).astype(np.uint32)

    def KeySwitchExt(self, c, stream=None):  # keyswitch-hybrid.cpp:217-243, one element
        out = self.ctx.empty(c.batch, c.n_limbs + self.sizeP, self.ext_limbs(c.n_limbs))
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_ext(self.h, c.ptr, c.n_limbs, c.batch, out.ptr, stream))
        return out

    def EvalFastRotationExt(self, key, c0, c1, k, add_first, stream=None):  # ckksrns-leveledshe.cpp:534-582 (digits in ws)
        ws, wsb = self.workspace(c0.n_limbs, c0.batch)
        idx = self.ext_limbs(c0.n_limbs)
        o0, o1 = (self.ctx.empty(c0.batch, len(idx), idx) for _ in range(2))
        self.ctx.lib.check(self.ctx.lib.L.fhe_eval_fast_rotation_ext(self.h, key, c0.ptr, c1.ptr, k, 1 if add_first else 0,
                                                                     c0.n_limbs, c0.batch, o0.ptr, o1.ptr, ws, wsb, stream))
        return o0, o1

    def KeySwitchDown(self, x0, x1, sizeQl, stream=None):  # keyswitch-hybrid.cpp:245-278
        ws, wsb = self.workspace(sizeQl, x0.batch)
        o0, o1 = self.ctx.empty(x0.batch, sizeQl), self.ctx.empty(x0.batch, sizeQl)
        self.ctx.lib.check(self.ctx.lib.L.fhe_ks_down(self.h, x0.ptr, x1.ptr, sizeQl, x0.batch, o0.ptr, o1.ptr, ws, wsb, stream))
        return o0, o1

    def BsgsTransform(self, c0, c1, in_rot, out_rot, diag, ws=None, out=None, stream=None):
        """fhe_ckks_bsgs_transform: in_rot / out_rot = lists of (automorphism index, key handle) or None for "no rotation";
        diag[i][j] = device pointer of the plaintext rows of outer step i, inner rotation j (None = absent).
        ws = (pointer, bytes) of a caller-owned workspace (needed for graph capture), else allocated per call."""
        L = self.ctx.lib.L
        nIn, nOut = len(in_rot), len(out_rot)

        def split(rots):
            ks = (C.c_uint32 * len(rots))(*[0 if r is None else int(r[0]) for r in rots])
            hs = (vp * len(rots))(*[None if r is None else r[1] for r in rots])
            return ks, hs
        inK, inH = split(in_rot)
        outK, outH = split(out_rot)
        dp = (vp * (nIn * nOut))(*[diag[i][j] for i in range(nOut) for j in range(nIn)])
        own = ws is None
        if own:
            wsb = L.fhe_ckks_bsgs_workspace_bytes(self.h, c0.n_limbs, c0.batch, nIn, nOut)
            ws = (self.ctx.malloc(wsb), wsb)
        o0, o1 = out if out is not None else (c0.like(), c0.like())
        self.ctx.lib.check(L.fhe_ckks_bsgs_transform(self.h, c0.ptr, c1.ptr, c0.n_limbs, c0.batch, nIn, inK, inH, nOut, outK,
                                                     outH, dp, o0.ptr, o1.ptr, ws[0], ws[1], stream))
        if own:
            self.ctx.sync(stream)
            self.ctx.free(ws[0])
        return o0, o1

    def EvalLinearTransform(self, A, c0, c1, bStep, rot_keys, stream=None):
        """FHECKKSRNS::EvalLinearTransform (ckksrns-fhe.cpp:1832-1882).  A = device pointers of the `slots` encoded diagonals
        (EvalLinearTransformPrecompute), rot_keys[index] = (automorphism index, key handle) for the baby steps 1..bStep-1
        and the giant steps bStep*j."""
        slots = len(A)
        gStep = -(-slots // bStep)
        in_rot = [None] + [rot_keys[i] for i in range(1, bStep)]
        out_rot = [None] + [rot_keys[bStep * j] for j in range(1, gStep)]
        diag = [[A[bStep * j + i] if bStep * j + i < slots else None for i in range(bStep)] for j in range(gStep)]
        return self.BsgsTransform(c0, c1, in_rot, out_rot, diag, stream=stream)

    def EvalAutomorphism(self, key, c0, c1, k, stream=None, t=0):  # base-leveledshe.cpp:381-422
        ws, wsb = self.workspace(c0.n_limbs, c0.batch)
        o0, o1 = c0.like(), c0.like()
        L = self.ctx.lib.L
        if t:
            self.ctx.lib.check(L.fhe_bgv_eval_automorphism(self.h, key, c0.ptr, c1.ptr, k, c0.n_limbs, t, c0.batch, o0.ptr, o1.ptr, ws,
                                                           wsb, stream))
        else:
            self.ctx.lib.check(L.fhe_eval_automorphism(self.h, key, c0.ptr, c1.ptr, k, c0.n_limbs, c0.batch, o0.ptr, o1.ptr, ws, wsb,
                                                       stream))
        return o0, o1

    def ApproxModDown(self, x, sizeQl, t=0, stream=None):  # dcrtpoly-impl.h:966-1005 (t > 0: the BGV form)
        ws, wsb = self.workspace(sizeQl, x.batch)
        out = self.ctx.empty(x.batch, sizeQl)
        L = self.ctx.lib.L
        if t:
            self.ctx.lib.check(L.fhe_approx_mod_down_bgv(self.h, x.ptr, sizeQl, t, x.batch, out.ptr, ws, wsb, stream))
        else:
            self.ctx.lib.check(L.fhe_approx_mod_down(self.h, x.ptr, sizeQl, x.batch, out.ptr, ws, wsb, stream))
        return out


class BvKey:
    """A BV evaluation key (KeySwitchBV, keyswitch-bv.cpp) over the context's leading sizeQ limbs with digit size base_bits: keyB / keyA
    are the key's b / a vectors, uint64 [D_0][sizeQ][N] in EVALUATION format, D_0 = digits(sizeQ).  The digits of the last Precompute stay
    in the key object's workspace (hoisting: one Precompute, FastKeySwitch with any key of the same base_bits via `ws_of`)."""

    def __init__(self, ctx, sizeQ, base_bits, keyB, keyA):
        self.ctx, self.sizeQ, self.base_bits = ctx, sizeQ, base_bits
        keyB = np.ascontiguousarray(keyB, dtype=np.uint64)
        keyA = np.ascontiguousarray(keyA, dtype=np.uint64)
        d0 = ctx.lib.L.fhe_crt_decompose_towers(ctx.h, None, sizeQ, base_bits)
        if d0 and (keyB.size != d0 * sizeQ * ctx.N or keyA.size != keyB.size):
            raise ValueError(f"a BV key of digit size {base_bits} over {sizeQ} limbs is uint64[{d0}][{sizeQ}][{ctx.N}] per vector")
        h = vp()
        ctx.lib.check(ctx.lib.L.fhe_bv_key_upload(ctx.h, sizeQ, base_bits, keyB.ctypes.data_as(u64p), keyA.ctypes.data_as(u64p),
                                                  C.byref(h)))
        self.h = h
        self._ws = None
        self._ws_bytes = 0

    def close(self):
        if self.h:
            self.ctx.lib.L.fhe_bv_key_destroy(self.h)
            self.h = None
        if self._ws is not None and self.ctx.h:
            self.ctx.free(self._ws)
        self._ws = None

    # ---- key generation on the device (KeySwitchBV::KeySwitchGenInternal, keyswitch-bv.cpp:49-225) ----
    @classmethod
    def wrap(cls, ctx, sizeQ, base_bits, dev_b, dev_a):
        """adopt device-resident key vectors [D_0][sizeQ][N] (fhe_bv_key_wrap): the memory stays with its owner"""
        self = cls.__new__(cls)
        self.ctx, self.sizeQ, self.base_bits = ctx, sizeQ, base_bits
        h = vp()
        ctx.lib.check(ctx.lib.L.fhe_bv_key_wrap(ctx.h, sizeQ, base_bits, vp(dev_b), vp(dev_a), C.byref(h)))
        self.h, self._ws, self._ws_bytes = h, None, 0
        return self

    @staticmethod
    def _towers(ctx, sizeQ, base_bits):
        """D_0; a digit size outside the device path raises the library's own error (FHE_ERR_UNSUPPORTED)"""
        d0 = ctx.lib.L.fhe_crt_decompose_towers(ctx.h, None, sizeQ, base_bits)
        if d0 == 0:
            na, ne = u64(), u64()
            ctx.lib.check(ctx.lib.L.fhe_bv_keygen_counters(ctx.h, sizeQ, base_bits, 1, 0, C.byref(na), C.byref(ne)))
        return d0

    @classmethod
    def _wrap_keys(cls, ctx, sizeQ, base_bits, b, a, n_keys, rotations):
        words = (b.batch // n_keys) * sizeQ * ctx.N
        keys = [cls.wrap(ctx, sizeQ, base_bits, b.ptr.value + 8 * words * i, a.ptr.value + 8 * words * i) for i in range(n_keys)]
        for k in keys:
            k._keep = (b, a)  # the slabs own the memory the handles point into
        return keys if rotations is None else dict(zip(rotations, keys))

    @staticmethod
    def _indices(ctx, n_keys, k_new, k_old, rotations):
        if rotations is not None:
            assert k_new is None and k_old is None and len(rotations) == n_keys
            k_new, k_old = rotation_key_indices(ctx.lib, rotations, ctx.N)
        kn, knp = _np_u32(k_new)
        ko, kop = _np_u32(k_old)
        assert (kn is None or len(kn) == n_keys) and (ko is None or len(ko) == n_keys)
        return (kn, ko), knp, kop

    @classmethod
    def keygen(cls, ctx, base_bits, s_new, s_old, a, e, n_keys=1, k_new=None, k_old=None, ns=1, rotations=None, in_place=False,
               stream=None):
        """fhe_bv_keygen with the caller's a and e, Towers [n_keys * D_0][sizeQ][N] in EVALUATION format; s_new, s_old [1][sizeQ][N].
        k_new / k_old: automorphism indices per key (None = 1), or rotations = rotation indices (rotation_key_indices).  in_place: b
        overwrites e.  Returns (b, a, keys): the two slabs and the wrapped BvKeys, a dict by rotation index when rotations were given."""
        sizeQ = a.n_limbs
        assert e.batch == a.batch and e.n_limbs == sizeQ and a.batch % n_keys == 0
        keep, knp, kop = cls._indices(ctx, n_keys, k_new, k_old, rotations)
        b = e if in_place else e.like()
        ctx.lib.check(ctx.lib.L.fhe_bv_keygen(ctx.h, sizeQ, base_bits, n_keys, knp, kop, s_new.ptr, s_old.ptr, ns, a.ptr, e.ptr, b.ptr,
                                              stream))
        return b, a, cls._wrap_keys(ctx, sizeQ, base_bits, b, a, n_keys, rotations)

    @classmethod
    def keygen_blake2(cls, ctx, base_bits, s_new, s_old, n_keys, key, counter_a, counter_e, k_new=None, k_old=None, ns=1, sigma=3.19,
                      rotations=None, stream=None):
        """fhe_bv_keygen_blake2: a = the uniform blake2 sampler's words from counter_a, e = the Gaussian sampler's from counter_e.
        Returns (b, a, keys) as keygen does."""
        sizeQ = s_new.n_limbs
        d0 = cls._towers(ctx, sizeQ, base_bits)
        keep, knp, kop = cls._indices(ctx, n_keys, k_new, k_old, rotations)
        b, a = ctx.empty(n_keys * d0, sizeQ), ctx.empty(n_keys * d0, sizeQ)
        kw = _key_words(key)
        ctx.lib.check(ctx.lib.L.fhe_bv_keygen_blake2(ctx.h, sizeQ, base_bits, n_keys, knp, kop, s_new.ptr, s_old.ptr, ns, sigma,
                                                     kw.ctypes.data_as(u32p), counter_a, counter_e, b.ptr, a.ptr, stream))
        return b, a, cls._wrap_keys(ctx, sizeQ, base_bits, b, a, n_keys, rotations)

    @classmethod
    def keygen_pk(cls, ctx, base_bits, pk_b, pk_a, s_old, u, e0, e1, n_keys=1, ns=1, in_place=False, stream=None):
        """fhe_bv_keygen_pk (the re-encryption key of PREBase::ReKeyGen): b = p0 * u + ns * e0 + factor * s_old, a = p1 * u + ns * e1 for
        Towers u, e0, e1 [n_keys * D_0][sizeQ][N]; pk_b, pk_a [1][sizeQ][N], or [n_keys][sizeQ][N] for one public key per key.
        in_place: b, a overwrite e0, e1.  Returns (b, a, keys)."""
        sizeQ = u.n_limbs
        assert e0.batch == u.batch == e1.batch and e0.n_limbs == e1.n_limbs == sizeQ and u.batch % n_keys == 0
        assert pk_b.batch == pk_a.batch and pk_b.batch in (1, n_keys) and pk_b.n_limbs == pk_a.n_limbs == sizeQ
        b, a = (e0, e1) if in_place else (e0.like(), e1.like())
        ctx.lib.check(ctx.lib.L.fhe_bv_keygen_pk(ctx.h, sizeQ, base_bits, n_keys, pk_b.ptr, pk_a.ptr, 1 if pk_b.batch > 1 else 0, s_old.ptr,
                                                 ns, u.ptr, e0.ptr, e1.ptr, b.ptr, a.ptr, stream))
        return b, a, cls._wrap_keys(ctx, sizeQ, base_bits, b, a, n_keys, None)

    @classmethod
    def keygen_pk_blake2(cls, ctx, base_bits, pk_b, pk_a, s_old, n_keys, key, counter_u, counter_e, ns=1, sigma=3.19, u_dist=0,
                         contiguous=True, stream=None):
        """fhe_bv_keygen_pk_blake2: u from counter_u, e0 and e1 from counter_e of the blake2 key.  contiguous: b, a and the workspace are
        one allocation (one Gaussian call and one transform); otherwise three.  Returns (b, a, keys): windows of one Tower that b owns
        when contiguous."""
        sizeQ = s_old.n_limbs
        d0 = cls._towers(ctx, sizeQ, base_bits)
        assert pk_b.batch == pk_a.batch and pk_b.batch in (1, n_keys) and pk_b.n_limbs == pk_a.n_limbs == sizeQ
        wsb = ctx.lib.L.fhe_bv_keygen_workspace_bytes(ctx.h, sizeQ, base_bits, n_keys)
        if contiguous:
            slab = ctx.empty(3 * n_keys * d0, sizeQ)
            b, a, ws = _window(slab, 0, n_keys * d0), _window(slab, n_keys * d0, n_keys * d0), vp(slab.ptr.value + 2 * wsb)
            b._keep = a._keep = slab
        else:
            b, a, spare = ctx.empty(n_keys * d0, sizeQ), ctx.empty(n_keys * d0, sizeQ), ctx.malloc(wsb + 16)
            ws = vp(spare.value + 16) if spare.value == a.ptr.value + wsb and a.ptr.value == b.ptr.value + wsb else spare
        kw = _key_words(key)
        try:
            ctx.lib.check(ctx.lib.L.fhe_bv_keygen_pk_blake2(ctx.h, sizeQ, base_bits, n_keys, pk_b.ptr, pk_a.ptr, 1 if pk_b.batch > 1 else 0,
                                                            s_old.ptr, u_dist, ns, sigma, kw.ctypes.data_as(u32p), counter_u, counter_e,
                                                            b.ptr, a.ptr, ws, wsb, stream))
            ctx.sync(stream)
        finally:
            if not contiguous:
                ctx.free(spare)
        return b, a, cls._wrap_keys(ctx, sizeQ, base_bits, b, a, n_keys, None)

    def digits(self, sizeQl):
        """D_l: towers of CRTDecompose(base_bits) at level sizeQl (the first D_l towers of the key)"""
        return self.ctx.lib.L.fhe_crt_decompose_towers(self.ctx.h, None, sizeQl, self.base_bits)

    def workspace(self, sizeQl, batch):
        need = self.ctx.lib.L.fhe_bv_workspace_bytes(self.ctx.h, sizeQl, self.base_bits, batch)
        if need > self._ws_bytes:
            if self._ws is not None:
                self.ctx.free(self._ws)
            self._ws = self.ctx.malloc(need)
            self._ws_bytes = need
        return self._ws, self._ws_bytes

    def Precompute(self, c, stream=None):  # keyswitch-bv.cpp:251-259: the digits [D_l][batch][sizeQl][N] at the start of the workspace
        ws, wsb = self.workspace(c.n_limbs, c.batch)
        self.ctx.lib.check(self.ctx.lib.L.fhe_bv_precompute(self.ctx.h, c.ptr, 1 if c.fmt == EVALUATION else 0, c.n_limbs, self.base_bits,
                                                            c.batch, ws, wsb, stream))
        return ws, wsb

    def FastKeySwitch(self, sizeQl, batch, acc0=None, acc1=None, ws_of=None, stream=None):  # keyswitch-bv.cpp:261-278
        """on the digits of the last Precompute of `ws_of` (default: this key); acc0 / acc1 given: acc += result, in place"""
        ws, wsb = (ws_of or self).workspace(sizeQl, batch)
        acc = acc0 is not None
        o0 = acc0 if acc else self.ctx.empty(batch, sizeQl)
        o1 = acc1 if acc else self.ctx.empty(batch, sizeQl)
        self.ctx.lib.check(self.ctx.lib.L.fhe_bv_fast_keyswitch(self.h, sizeQl, batch, o0.ptr, o1.ptr, 1 if acc else 0, ws, wsb, stream))
        return o0, o1

    def KeySwitchCore(self, c, acc0=None, acc1=None, stream=None):  # keyswitch-bv.cpp:245-249 (+ base-leveledshe.cpp:207-211 with acc)
        ws, wsb = self.workspace(c.n_limbs, c.batch)
        acc = acc0 is not None
        o0 = acc0 if acc else c.like()
        o1 = acc1 if acc else c.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_keyswitch_bv(self.h, c.ptr, c.n_limbs, c.batch, o0.ptr, o1.ptr, 1 if acc else 0, ws, wsb,
                                                           stream))
        return o0, o1

    def FastRotation(self, c0, k, ws_of=None, stream=None):  # base-leveledshe.cpp:432-463
        """(Auto_k(c0 + ks0), Auto_k(ks1)) on the digits the last Precompute(c1) of `ws_of` (default: this key) left; k = automorphism index"""
        ws, wsb = (ws_of or self).workspace(c0.n_limbs, c0.batch)
        o0, o1 = c0.like(), c0.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_bv_eval_fast_rotation(self.h, c0.ptr, k, c0.n_limbs, c0.batch, o0.ptr, o1.ptr, ws, wsb, stream))
        return o0, o1

    def Automorphism(self, c0, c1, k, stream=None):  # base-leveledshe.cpp:381-422
        ws, wsb = self.workspace(c0.n_limbs, c0.batch)
        o0, o1 = c0.like(), c0.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_bv_eval_automorphism(self.h, c0.ptr, c1.ptr, k, c0.n_limbs, c0.batch, o0.ptr, o1.ptr, ws, wsb,
                                                                   stream))
        return o0, o1


def rotation_key_indices(lib, rotations, N):
    """(kNew, kOld) of the evaluation keys of CKKS rotations (LeveledSHEBase::EvalAutomorphismKeyGen, base-leveledshe.cpp:336-379): for
    the automorphism index k = FindAutomorphismIndex2nComplex(rotation) the key switches sigma_{k^-1}(s) ... to s, i.e. the NEW secret is
    the permuted one (kNew = k^-1 mod 2N) and the old one is s itself (kOld = 1)"""
    ks = [lib.find_automorphism_index(int(r), 2 * N) for r in rotations]
    return np.array([pow(k, -1, 2 * N) for k in ks], np.uint32), np.ones(len(ks), np.uint32)


SECRET_KEY_FORM, PUBLIC_KEY_FORM = 0, 1  # form of bv_keygen_counters


def bv_keygen_counters(ctx, sizeQ, base_bits, n_keys, form=SECRET_KEY_FORM):
    """(blake2 counters a seeded BV key generation consumes from counter_a or counter_u, from counter_e) (fhe_bv_keygen_counters)"""
    n0, ne = u64(), u64()
    ctx.lib.check(ctx.lib.L.fhe_bv_keygen_counters(ctx.h, sizeQ, base_bits, n_keys, form, C.byref(n0), C.byref(ne)))
    return n0.value, ne.value


def bv_keygen_factors(qs, base_bits):
    """The factor table of a BV key with plain integers: rows = towers in the order of CRTDecompose (limb 0's windows, least significant
    first, then limb 1's ...), factor[d][i] = 2^(base_bits * k) mod q_i when tower d is window k of limb i, else 0; base_bits == 0: one
    tower per limb with factor 1 (host::bv_keygen_factors, csrc/host_math.h)"""
    qs = [int(q) for q in qs]
    rows = []
    for i, q in enumerate(qs):
        for k in range(-(-q.bit_length() // base_bits) if base_bits else 1):
            rows.append([pow(2, base_bits * k, q) if j == i else 0 for j in range(len(qs))])
    return rows


def keygen_combine(ctx, a, e, s_new, n_keys=1, k_new=None, s_old=None, k_old=None, factor=None, ns=1, out=None, stream=None):
    """fhe_keygen_combine over the limbs of `a`: a, e Towers [n_keys * nParts][nLimbs][N], s_new / s_old [1][nLimbs][N], factor
    [nParts][nLimbs] (None: no s_old term); out: a Tower to write (e itself = in place), default a new one"""
    n_parts, rem = divmod(a.batch, n_keys)
    assert rem == 0 and e.batch == a.batch and e.n_limbs == a.n_limbs
    kn, knp = _np_u32(k_new)
    ko, kop = _np_u32(k_old)
    f = fp = None
    if factor is not None:
        f = np.ascontiguousarray(np.asarray(factor, dtype=np.uint64))
        assert f.shape == (n_parts, a.n_limbs)
        fp = f.ctypes.data_as(u64p)
    out = a.like() if out is None else out
    ctx.lib.check(ctx.lib.L.fhe_keygen_combine(ctx.h, a._li(), a.n_limbs, n_keys, n_parts, a.ptr, e.ptr, s_new.ptr, knp,
                                               None if s_old is None else s_old.ptr, kop, fp, ns, out.ptr, stream))
    return out


def public_key(ctx, s, a, e, ns=1, stream=None):
    """PKEBase::KeyGenInternal (base-pke.cpp:47-98): b = ns * e - a * s for towers [batch][nLimbs][N] in EVALUATION format, one public
    key per tower of the batch against the one secret s [1][nLimbs][N]; returns b (a is the other half)"""
    return keygen_combine(ctx, a, e, s, n_keys=a.batch, ns=ns, stream=stream)


TERNARY, GAUSSIAN = 0, 1  # vDist of encrypt_pk_blake2: the distribution of v (SecretKeyDist != GAUSSIAN / == GAUSSIAN, rns-pke.cpp:164-165)
PUBLIC_KEY, SECRET_KEY = 0, 1  # form of encrypt_counters


def _window(t, first, batch):
    """towers [first, first + batch) of the Tower t, not owned"""
    return Tower(t.ctx, vp(t.ptr.value + 8 * first * t.n_limbs * t.ctx.N), batch, t.n_limbs, t.limb_idx, t.fmt)


def encrypt_pk_combine(ctx, pk_b, pk_a, v, e0, e1, msg=None, ns=1, in_place=False, stream=None):
    """fhe_encrypt_pk_combine over the limbs of v: c0 = pkB * v + ns * e0 (+ msg), c1 = pkA * v + ns * e1 for Towers [batch][nLimbs][N] in
    EVALUATION format; pk_b, pk_a [1][>= nLimbs][N] (their first nLimbs rows are used).  Returns (c0, c1): new Towers, or e0 and e1
    themselves with in_place"""
    assert e0.batch == v.batch == e1.batch and e0.n_limbs == v.n_limbs == e1.n_limbs and pk_b.n_limbs >= v.n_limbs <= pk_a.n_limbs
    c0, c1 = (e0, e1) if in_place else (e0.like(), e1.like())
    ctx.lib.check(ctx.lib.L.fhe_encrypt_pk_combine(ctx.h, v._li(), v.n_limbs, v.batch, pk_b.ptr, pk_a.ptr, v.ptr, e0.ptr, e1.ptr,
                                                   None if msg is None else msg.ptr, ns, c0.ptr, c1.ptr, stream))
    return c0, c1


def encrypt_sk_combine(ctx, s, a, e, msg=None, ns=1, in_place=False, stream=None):
    """fhe_encrypt_sk_combine over the limbs of a: c0 = a * s + ns * e (+ msg), c1 = -a; s [1][>= nLimbs][N].  Returns (c0, c1): new
    Towers, or e and a themselves with in_place"""
    assert e.batch == a.batch and e.n_limbs == a.n_limbs <= s.n_limbs
    c0, c1 = (e, a) if in_place else (e.like(), a.like())
    ctx.lib.check(ctx.lib.L.fhe_encrypt_sk_combine(ctx.h, a._li(), a.n_limbs, a.batch, s.ptr, a.ptr, e.ptr, None if msg is None else msg.ptr,
                                                   ns, c0.ptr, c1.ptr, stream))
    return c0, c1


def encrypt_counters(ctx, n_limbs, batch, form=PUBLIC_KEY):
    """(blake2 counters a seeded call consumes from counter_v or counter_a, from counter_e) (fhe_encrypt_counters)"""
    n0, ne = C.c_uint64(), C.c_uint64()
    ctx.lib.check(ctx.lib.L.fhe_encrypt_counters(ctx.h, n_limbs, batch, form, C.byref(n0), C.byref(ne)))
    return n0.value, ne.value


def encrypt_pk_blake2(ctx, pk_b, pk_a, batch, key, counter_v, counter_e, n_limbs=None, limb_idx=None, msg=None, ns=1, sigma=3.19,
                      v_dist=TERNARY, contiguous=True, stream=None):
    """fhe_encrypt_pk_blake2: `batch` fresh ciphertexts under the public key (pk_b, pk_a) at the level of n_limbs rows (default: the
    key's), v from counter_v and e0 ‖ e1 from counter_e of the blake2 key; msg: a Tower [batch][nLimbs][N] in either format, or None.
    contiguous: the workspace follows the ciphertexts in one allocation (one forward transform instead of two).  Returns (c0, c1), windows
    of one Tower that c0 owns."""
    n_limbs = pk_b.n_limbs if n_limbs is None else n_limbs
    li = pk_b.limb_idx if limb_idx is None else limb_idx
    wsb = ctx.lib.L.fhe_encrypt_workspace_bytes(ctx.h, n_limbs, batch)
    ct = ctx.empty((3 if contiguous else 2) * batch, n_limbs, li)
    ws = spare = vp(ct.ptr.value + 2 * wsb) if contiguous else ctx.malloc(wsb + 16)
    if not contiguous and ws.value == ct.ptr.value + 2 * wsb:  # the allocator put it right behind ct: step off, "apart" is what was asked for
        ws = vp(spare.value + 16)
    k = _key_words(key)
    try:
        ctx.lib.check(ctx.lib.L.fhe_encrypt_pk_blake2(ctx.h, ct._li(), n_limbs, batch, pk_b.ptr, pk_a.ptr, v_dist, ns, sigma,
                                                      k.ctypes.data_as(u32p), counter_v, counter_e, None if msg is None else msg.ptr,
                                                      EVALUATION if msg is None else msg.fmt, ct.ptr, ws, wsb, stream))
        ctx.sync(stream)
    finally:
        if not contiguous:
            ctx.free(spare)
    c0, c1 = _window(ct, 0, batch), _window(ct, batch, batch)
    c0._keep = c1._keep = ct
    return c0, c1


def encrypt_sk_blake2(ctx, s, batch, key, counter_a, counter_e, n_limbs=None, limb_idx=None, msg=None, ns=1, sigma=3.19, stream=None):
    """fhe_encrypt_sk_blake2: `batch` fresh ciphertexts under the secret key s, a from counter_a (the c1 half is minus the uniform
    sampler's words) and e from counter_e.  Returns (c0, c1) as encrypt_pk_blake2 does."""
    n_limbs = s.n_limbs if n_limbs is None else n_limbs
    ct = ctx.empty(2 * batch, n_limbs, s.limb_idx if limb_idx is None else limb_idx)
    k = _key_words(key)
    ctx.lib.check(ctx.lib.L.fhe_encrypt_sk_blake2(ctx.h, ct._li(), n_limbs, batch, s.ptr, ns, sigma, k.ctypes.data_as(u32p), counter_a,
                                                  counter_e, None if msg is None else msg.ptr, EVALUATION if msg is None else msg.fmt,
                                                  ct.ptr, stream))
    c0, c1 = _window(ct, 0, batch), _window(ct, batch, batch)
    c0._keep = c1._keep = ct
    return c0, c1


def _bfv_scaled(ctx, ptxt, t, neg_q_mod_t, t_inv_mod_q, stream):
    """DCRTPoly::TimesQovert (dcrtpoly-impl.h:868-885) of a COEFFICIENT plaintext Tower: the message PKEBFVRNS::Encrypt adds"""
    assert ptxt.fmt == COEFFICIENT
    tinv = np.ascontiguousarray(np.asarray(t_inv_mod_q, dtype=np.uint64))
    out = ptxt.like()
    ctx.lib.check(ctx.lib.L.fhe_times_q_over_t(ctx.h, out.ptr, ptxt.ptr, t, neg_q_mod_t, tinv.ctypes.data_as(u64p), ptxt._li(),
                                               ptxt.n_limbs, ptxt.batch, stream))
    return out


def bfv_encrypt_pk_blake2(ctx, pk_b, pk_a, ptxt, t, neg_q_mod_t, t_inv_mod_q, key, counter_v, counter_e, sigma=3.19, v_dist=TERNARY,
                          contiguous=True, stream=None):
    """PKEBFVRNS::Encrypt(ptxt, publicKey) with the STANDARD encryption technique (bfvrns-pke.cpp:157-213): fhe_times_q_over_t on the
    COEFFICIENT plaintext Tower [batch][sizeQl][N] (neg_q_mod_t = GetNegQModt(level), t_inv_mod_q = GettInvModq()), then the seeded call
    with the scaled message in COEFFICIENT format (it joins e0 before the forward transform)"""
    m = _bfv_scaled(ctx, ptxt, t, neg_q_mod_t, t_inv_mod_q, stream)
    return encrypt_pk_blake2(ctx, pk_b, pk_a, ptxt.batch, key, counter_v, counter_e, n_limbs=ptxt.n_limbs, limb_idx=ptxt.limb_idx, msg=m,
                             sigma=sigma, v_dist=v_dist, contiguous=contiguous, stream=stream)


def bfv_encrypt_sk_blake2(ctx, s, ptxt, t, neg_q_mod_t, t_inv_mod_q, key, counter_a, counter_e, sigma=3.19, stream=None):
    """PKEBFVRNS::Encrypt(ptxt, privateKey), STANDARD (bfvrns-pke.cpp:99-155), as bfv_encrypt_pk_blake2"""
    m = _bfv_scaled(ctx, ptxt, t, neg_q_mod_t, t_inv_mod_q, stream)
    return encrypt_sk_blake2(ctx, s, ptxt.batch, key, counter_a, counter_e, n_limbs=ptxt.n_limbs, limb_idx=ptxt.limb_idx, msg=m,
                             sigma=sigma, stream=stream)


def rescale(ctx, x, stream=None):
    """DCRTPoly::DropLastElementAndScale on a Tower over context limbs [0, sizeQl) (dcrtpoly-impl.h:693-712)."""
    sizeQl = x.n_limbs
    need = ctx.lib.L.fhe_rescale_workspace_bytes(ctx.h, sizeQl, x.batch)
    ws = ctx.malloc(need)
    out = ctx.empty(x.batch, sizeQl - 1)
    ctx.lib.check(ctx.lib.L.fhe_rescale(ctx.h, x.ptr, sizeQl, x.batch, out.ptr, ws, need, stream))
    ctx.sync(stream)
    ctx.free(ws)
    return out


def rescale_limbs(ctx, x, scale_tab, inv_tab, stream=None):
    """DropLastElementAndScale on a Tower over ANY limbs of the context (x.limb_idx; its last limb is dropped) with the caller's tables
    QlQlInvModqlDivqlModq / qlInvModq (dcrtpoly-impl.h:693-694), the entry the DCRTPoly backend calls."""
    sizeQl = x.n_limbs
    need = ctx.lib.L.fhe_rescale_workspace_bytes(ctx.h, sizeQl, x.batch)
    ws = ctx.malloc(need)
    kept = None if x.limb_idx is None else x.limb_idx[:sizeQl - 1]
    out = ctx.empty(x.batch, sizeQl - 1, kept)
    a = np.ascontiguousarray(scale_tab, dtype=np.uint64)
    b = np.ascontiguousarray(inv_tab, dtype=np.uint64)
    ctx.lib.check(ctx.lib.L.fhe_rescale_limbs(ctx.h, x.ptr, x._li(), sizeQl, a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), x.batch,
                                              out.ptr, ws, need, stream))
    ctx.sync(stream)
    ctx.free(ws)
    return out


def rescale_limbs_pair(ctx, x0, x1, scale_tab, inv_tab, stream=None):
    """the two elements of a ciphertext (two Towers of batch 1, allocated on their own) through fhe_rescale_limbs_pair"""
    sizeQl = x0.n_limbs
    need = ctx.lib.L.fhe_rescale_workspace_bytes(ctx.h, sizeQl, 2)
    ws = ctx.malloc(need)
    kept = None if x0.limb_idx is None else x0.limb_idx[:sizeQl - 1]
    o0, o1 = ctx.empty(1, sizeQl - 1, kept), ctx.empty(1, sizeQl - 1, kept)
    a = np.ascontiguousarray(scale_tab, dtype=np.uint64)
    b = np.ascontiguousarray(inv_tab, dtype=np.uint64)
    ctx.lib.check(ctx.lib.L.fhe_rescale_limbs_pair(ctx.h, x0.ptr, x1.ptr, x0._li(), sizeQl, a.ctypes.data_as(u64p), b.ctypes.data_as(u64p),
                                                   o0.ptr, o1.ptr, ws, need, stream))
    ctx.sync(stream)
    ctx.free(ws)
    return o0, o1


def _u64_or_null(v):
    if v is None:
        return None, None
    a = np.ascontiguousarray(v, dtype=np.uint64)
    return a, a.ctypes.data_as(u64p)


def rescale_multi(ctx, x, levels, n_out=None, scale=None, stream=None):
    """LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, levels) (ckksrns-leveledshe.cpp:172-191) on a Tower over context limbs [0, sizeQl)
    in one fused pass: optionally times the scalar's residues scale[sizeQl] first, the last `levels` limbs dropped and scaled, the first
    n_out limbs (default: all sizeQl - levels) produced."""
    sizeQl = x.n_limbs
    n_out = sizeQl - levels if n_out is None else n_out
    need = ctx.lib.L.fhe_rescale_multi_workspace_bytes(ctx.h, sizeQl, levels, x.batch)
    ws = ctx.malloc(max(need, 8))
    out = ctx.empty(x.batch, max(n_out, 1))
    sc, scp = _u64_or_null(scale)
    try:
        ctx.lib.check(ctx.lib.L.fhe_rescale_multi(ctx.h, x.ptr, sizeQl, levels, n_out, scp, x.batch, out.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return out


def rescale_multi_limbs(ctx, x, levels, scale_tabs, inv_tabs, n_out=None, scale=None, stream=None):
    """the same on a Tower over ANY limbs of the context (x.limb_idx; its last limbs are dropped, the last one first) with the caller's
    tables: scale_tabs / inv_tabs hold step k's QlQlInvModqlDivqlModq / qlInvModq (sizeQl-1-k residues) one after the other."""
    sizeQl = x.n_limbs
    n_out = sizeQl - levels if n_out is None else n_out
    need = ctx.lib.L.fhe_rescale_multi_workspace_bytes(ctx.h, sizeQl, levels, x.batch)
    ws = ctx.malloc(max(need, 8))
    kept = None if x.limb_idx is None else x.limb_idx[:n_out]
    out = ctx.empty(x.batch, max(n_out, 1), kept)
    a, ap = _u64_or_null(scale_tabs)
    b, bp = _u64_or_null(inv_tabs)
    sc, scp = _u64_or_null(scale)
    try:
        ctx.lib.check(ctx.lib.L.fhe_rescale_multi_limbs(ctx.h, x.ptr, x._li(), sizeQl, levels, n_out, scp, ap, bp, x.batch, out.ptr, ws,
                                                        need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return out


def rescale_multi_pair(ctx, x0, x1, levels, scale_tabs, inv_tabs, n_out=None, scale=None, stream=None):
    """the two elements of a ciphertext (two Towers of batch 1, allocated on their own) through fhe_rescale_multi_limbs_pair"""
    sizeQl = x0.n_limbs
    n_out = sizeQl - levels if n_out is None else n_out
    need = ctx.lib.L.fhe_rescale_multi_workspace_bytes(ctx.h, sizeQl, levels, 2)
    ws = ctx.malloc(max(need, 8))
    kept = None if x0.limb_idx is None else x0.limb_idx[:n_out]
    o0, o1 = ctx.empty(1, max(n_out, 1), kept), ctx.empty(1, max(n_out, 1), kept)
    a, ap = _u64_or_null(scale_tabs)
    b, bp = _u64_or_null(inv_tabs)
    sc, scp = _u64_or_null(scale)
    try:
        ctx.lib.check(ctx.lib.L.fhe_rescale_multi_limbs_pair(ctx.h, x0.ptr, x1.ptr, x0._li(), sizeQl, levels, n_out, scp, ap, bp, o0.ptr,
                                                             o1.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return o0, o1


def lincomb(ctx, towers, consts, accumulate_into=None, stream=None):
    """fhe_lincomb: sum_i consts[i] (.) towers[i] per limb (pke's weighted sum, ckksrns-advancedshe.cpp:97-136) in one launch per 16 terms;
    consts[i][r] = the constant of term i on limb r (reduced).  accumulate_into: a Tower the sum is added to (returned), else a new one."""
    t0 = towers[0]
    out = accumulate_into if accumulate_into is not None else ctx.empty(t0.batch, t0.n_limbs, t0.limb_idx, t0.fmt)
    ptrs = (vp * len(towers))(*[t.ptr.value if hasattr(t.ptr, "value") else t.ptr for t in towers])
    k = np.ascontiguousarray(consts, dtype=np.uint64).reshape(len(towers), t0.n_limbs)
    ctx.lib.check(ctx.lib.L.fhe_lincomb(ctx.h, out.ptr, ptrs, k.ctypes.data_as(u64p), len(towers), t0._li(), t0.n_limbs, t0.batch,
                                         1 if accumulate_into is not None else 0, stream))
    ctx.sync(stream)
    return out


def elem_pair(ctx, kind, a0, a1, b0=None, b1=None, consts=None, in_place=False, stream=None):
    """fhe_add_pair / fhe_sub_pair / fhe_mul_const_pair on Towers of batch 1 allocated on their own"""
    n = a0.n_limbs
    o0, o1 = (a0, a1) if in_place else (ctx.empty(1, n, a0.limb_idx, a0.fmt), ctx.empty(1, n, a0.limb_idx, a0.fmt))
    if kind == "mul_const":
        k = np.ascontiguousarray(consts, dtype=np.uint64)
        ctx.lib.check(ctx.lib.L.fhe_mul_const_pair(ctx.h, o0.ptr, o1.ptr, a0.ptr, a1.ptr, k.ctypes.data_as(u64p), a0._li(), n, stream))
    else:
        f = ctx.lib.L.fhe_add_pair if kind == "add" else ctx.lib.L.fhe_sub_pair
        ctx.lib.check(f(ctx.h, o0.ptr, o1.ptr, a0.ptr, a1.ptr, b0.ptr, b1.ptr, a0._li(), n, stream))
    ctx.sync(stream)
    return o0, o1


def mod_reduce(ctx, x, t, stream=None):
    """DCRTPoly::ModReduce (BGV modulus switch by the last limb, dcrtpoly-impl.h:736-755) on a Tower over limbs [0, sizeQl)."""
    sizeQl = x.n_limbs
    need = ctx.lib.L.fhe_rescale_workspace_bytes(ctx.h, sizeQl, x.batch)
    ws = ctx.malloc(need)
    out = ctx.empty(x.batch, sizeQl - 1, None, x.fmt)
    ctx.lib.check(ctx.lib.L.fhe_mod_reduce(ctx.h, x.ptr, sizeQl, t, 1 if x.fmt == EVALUATION else 0, x.batch, out.ptr, ws,
                                           need, stream))
    ctx.sync(stream)
    ctx.free(ws)
    return out


def mod_reduce_limbs(ctx, x, t, negt_inv_modq, ql_inv_modq, stream=None):
    """DCRTPoly::ModReduce on a Tower over ANY limbs of the context (x.limb_idx; its last limb is dropped) with the caller's tables
    negtInvModq / qlInvModq (dcrtpoly-impl.h:736-738): fhe_mod_reduce_limbs, the entry the DCRTPoly backend calls."""
    sizeQl = x.n_limbs
    need = ctx.lib.L.fhe_rescale_workspace_bytes(ctx.h, sizeQl, x.batch)
    ws = ctx.malloc(need)
    kept = None if x.limb_idx is None else x.limb_idx[:sizeQl - 1]
    out = ctx.empty(x.batch, sizeQl - 1, kept, x.fmt)
    b = np.ascontiguousarray(ql_inv_modq, dtype=np.uint64)
    try:
        ctx.lib.check(ctx.lib.L.fhe_mod_reduce_limbs(ctx.h, x.ptr, x._li(), sizeQl, t, negt_inv_modq, b.ctypes.data_as(u64p),
                                                     1 if x.fmt == EVALUATION else 0, x.batch, out.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return out


def mod_reduce_pair(ctx, x0, x1, t, negt_inv_modq, ql_inv_modq, stream=None):
    """the two elements of a ciphertext (two Towers of batch 1, allocated on their own) through fhe_mod_reduce_limbs_pair"""
    sizeQl = x0.n_limbs
    need = ctx.lib.L.fhe_rescale_workspace_bytes(ctx.h, sizeQl, 2)
    ws = ctx.malloc(need)
    kept = None if x0.limb_idx is None else x0.limb_idx[:sizeQl - 1]
    o0, o1 = ctx.empty(1, sizeQl - 1, kept, x0.fmt), ctx.empty(1, sizeQl - 1, kept, x0.fmt)
    b = np.ascontiguousarray(ql_inv_modq, dtype=np.uint64)
    try:
        ctx.lib.check(ctx.lib.L.fhe_mod_reduce_limbs_pair(ctx.h, x0.ptr, x1.ptr, x0._li(), sizeQl, t, negt_inv_modq, b.ctypes.data_as(u64p),
                                                          1 if x0.fmt == EVALUATION else 0, o0.ptr, o1.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return o0, o1


def _drop_rows(sizeQl, levels, drop_rows):
    """(levels, the row list and its ctypes pointer or None, the lowest dropped row)"""
    if drop_rows is None:
        return levels, None, None, sizeQl - levels
    rows = np.ascontiguousarray(drop_rows, dtype=np.uint32)
    return len(rows), rows, rows.ctypes.data_as(u32p), int(rows[-1]) if len(rows) else 0


def mod_reduce_multi(ctx, x, t, levels=1, scalar=1, drop_rows=None, n_out=None, stream=None):
    """The level alignment of BGV's automatic scaling modes on one operand (LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace,
    bgvrns-leveledshe.cpp:83-233) as one call, fhe_mod_reduce_multi: every row of a Tower over context limbs [0, sizeQl) times `scalar`, then
    DCRTPoly::ModReduce on the rows drop_rows (strictly decreasing; None: the last `levels` rows) with the rows above each discarded, of
    which the first n_out rows (default: all below the lowest dropped row) are produced."""
    sizeQl = x.n_limbs
    levels, rows, rp, lowest = _drop_rows(sizeQl, levels, drop_rows)
    n_out = lowest if n_out is None else n_out
    need = ctx.lib.L.fhe_mod_reduce_multi_workspace_bytes(ctx.h, sizeQl, levels, x.batch)
    ws = ctx.malloc(max(need, 8))
    out = ctx.empty(x.batch, max(n_out, 1), None, x.fmt)
    try:
        ctx.lib.check(ctx.lib.L.fhe_mod_reduce_multi(ctx.h, x.ptr, sizeQl, t, scalar, rp, levels, n_out, 1 if x.fmt == EVALUATION else 0,
                                                     x.batch, out.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return out


def mod_reduce_multi_limbs(ctx, x, t, negt_inv_modq, ql_inv_modq, levels=1, scalar=1, drop_rows=None, n_out=None, stream=None):
    """the same on a Tower over ANY limbs of the context (x.limb_idx) with the caller's tables: negt_inv_modq[k] and, one after the other,
    step k's drop_rows[k] residues of qlInvModq (CryptoParametersBGVRNS::GetNegtInvModq / GetqlInvModq of that row)."""
    sizeQl = x.n_limbs
    levels, rows, rp, lowest = _drop_rows(sizeQl, levels, drop_rows)
    n_out = lowest if n_out is None else n_out
    need = ctx.lib.L.fhe_mod_reduce_multi_workspace_bytes(ctx.h, sizeQl, levels, x.batch)
    ws = ctx.malloc(max(need, 8))
    kept = None if x.limb_idx is None else x.limb_idx[:n_out]
    out = ctx.empty(x.batch, max(n_out, 1), kept, x.fmt)
    a, ap = _u64_or_null(negt_inv_modq)
    b, bp = _u64_or_null(ql_inv_modq)
    try:
        ctx.lib.check(ctx.lib.L.fhe_mod_reduce_multi_limbs(ctx.h, x.ptr, x._li(), sizeQl, t, scalar, rp, levels, n_out, ap, bp,
                                                           1 if x.fmt == EVALUATION else 0, x.batch, out.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return out


def mod_reduce_multi_pair(ctx, x0, x1, t, negt_inv_modq, ql_inv_modq, levels=1, scalar=1, drop_rows=None, n_out=None, stream=None):
    """the two elements of a ciphertext (two Towers of batch 1, allocated on their own) through fhe_mod_reduce_multi_limbs_pair"""
    sizeQl = x0.n_limbs
    levels, rows, rp, lowest = _drop_rows(sizeQl, levels, drop_rows)
    n_out = lowest if n_out is None else n_out
    need = ctx.lib.L.fhe_mod_reduce_multi_workspace_bytes(ctx.h, sizeQl, levels, 2)
    ws = ctx.malloc(max(need, 8))
    kept = None if x0.limb_idx is None else x0.limb_idx[:n_out]
    o0, o1 = ctx.empty(1, max(n_out, 1), kept, x0.fmt), ctx.empty(1, max(n_out, 1), kept, x0.fmt)
    a, ap = _u64_or_null(negt_inv_modq)
    b, bp = _u64_or_null(ql_inv_modq)
    try:
        ctx.lib.check(ctx.lib.L.fhe_mod_reduce_multi_limbs_pair(ctx.h, x0.ptr, x1.ptr, x0._li(), sizeQl, t, scalar, rp, levels, n_out, ap, bp,
                                                                1 if x0.fmt == EVALUATION else 0, o0.ptr, o1.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        ctx.free(ws)
    return o0, o1


def mod_reduce_multi_tables(qs, t, drop_rows):
    """the tables fhe_mod_reduce_multi_limbs takes, as CryptoParametersBGVRNS holds them for a tower over moduli qs: negtInvModq of every
    dropped row and, one after the other, the rows' qlInvModq"""
    negt, inv = [], []
    for r in drop_rows:
        ql = int(qs[r])
        negt.append((-pow(t % ql, -1, ql)) % ql)
        inv += [pow(ql % int(qs[i]), -1, int(qs[i])) for i in range(r)]
    return np.array(negt, np.uint64), np.array(inv, np.uint64)


class BgvOperand:
    """what AdjustLevelsAndDepthInPlace reads of a ciphertext, and what bgv_adjust_plan decides for it: `scalar` (1: none), drop_rows (the
    rows ModReduce is called on, strictly decreasing) and n_out (the rows that are left)"""

    def __init__(self, level, noise_scale_deg, size_ql, scaling_factor_int):
        self.level, self.noise_scale_deg, self.size_ql, self.scaling_factor_int = level, noise_scale_deg, size_ql, int(scaling_factor_int)
        self.scalar, self.drop_rows, self.n_out = 1, [], size_ql

    def untouched(self):
        return self.scalar == 1 and not self.drop_rows and self.n_out == self.size_ql

    # the three members, as bookkeeping (bgvrns-leveledshe.cpp:44-81, 235-247)
    def _eval_mult_core(self, scalar, t):
        assert self.scalar == 1 and not self.drop_rows and self.n_out == self.size_ql, "the scalar product comes first"
        self.scalar = int(scalar)
        self.noise_scale_deg += 1
        self.scaling_factor_int = self.scaling_factor_int * int(scalar) % t

    def _mod_reduce(self, t, mod_reduce_factor_int):
        r = self.n_out - 1
        assert r >= 1, "Too few towers to support ModReduce."
        self.drop_rows.append(r)
        self.n_out, self.level, self.noise_scale_deg = r, self.level + 1, self.noise_scale_deg - 1
        self.scaling_factor_int = self.scaling_factor_int * pow(int(mod_reduce_factor_int[r]) % t, -1, t) % t

    def _level_reduce(self, levels):
        self.n_out, self.level = self.n_out - levels, self.level + levels


def bgv_adjust_plan(ct1, ct2, t, mod_reduce_factor_int, scaling_factor_int_big, to_one=False):
    """LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace (bgvrns-leveledshe.cpp:83-224; to_one: AdjustLevelsAndDepthToOneInPlace, :226-233) under
    FLEXIBLEAUTO / FLEXIBLEAUTOEXT as a plan: nothing touches a device.  ct1 / ct2: (level, noiseScaleDeg, sizeQl, scalingFactorInt);
    mod_reduce_factor_int[i] = GetModReduceFactorInt(i), scaling_factor_int_big[i] = GetScalingFactorIntBig(i).  Returns two BgvOperand with
    the new (level, noise_scale_deg, scaling_factor_int) and the (scalar, drop_rows, n_out) that bgv_adjust runs."""
    a, b = BgvOperand(*ct1), BgvOperand(*ct2)
    mrf, big = mod_reduce_factor_int, scaling_factor_int_big
    inv = lambda v: pow(int(v) % t, -1, t)
    if a.level != b.level:
        lo, hi = (a, b) if a.level < b.level else (b, a)  # the branches for c1lvl > c2lvl are those for c1lvl < c2lvl with the names swapped
        gap = hi.level - lo.level
        if lo.noise_scale_deg == 2:
            if hi.noise_scale_deg == 2:
                lo._eval_mult_core(hi.scaling_factor_int * inv(lo.scaling_factor_int) % t * (int(mrf[lo.size_ql - 1]) % t) % t, t)
                lo._mod_reduce(t, mrf)
                if gap > 1:
                    lo._level_reduce(gap - 1)
                lo.scaling_factor_int = hi.scaling_factor_int
            elif gap == 1:
                lo._mod_reduce(t, mrf)
            else:
                lo._eval_mult_core(int(big[hi.level - 1]) % t * inv(lo.scaling_factor_int) % t * (int(mrf[lo.size_ql - 1]) % t) % t, t)
                lo._mod_reduce(t, mrf)
                if gap > 2:
                    lo._level_reduce(gap - 2)
                lo._mod_reduce(t, mrf)
                lo.scaling_factor_int = hi.scaling_factor_int
        elif hi.noise_scale_deg == 2:
            lo._eval_mult_core(hi.scaling_factor_int * inv(lo.scaling_factor_int) % t, t)
            lo._level_reduce(gap)
            lo.scaling_factor_int = hi.scaling_factor_int
        else:
            lo._eval_mult_core(int(big[hi.level - 1]) % t * inv(lo.scaling_factor_int) % t, t)
            if gap > 1:
                lo._level_reduce(gap - 1)
            lo._mod_reduce(t, mrf)
            lo.scaling_factor_int = hi.scaling_factor_int
    elif a.noise_scale_deg < b.noise_scale_deg:
        a._eval_mult_core(a.scaling_factor_int, t)
    elif b.noise_scale_deg < a.noise_scale_deg:
        b._eval_mult_core(b.scaling_factor_int, t)
    if to_one and a.noise_scale_deg == 2:
        a._mod_reduce(t, mrf)
        b._mod_reduce(t, mrf)
    return a, b


def bgv_adjust(ctx, c0, c1, plan, t, qs=None, stream=None):
    """run one operand's plan on the two elements of its ciphertext (Towers of batch 1, allocated on their own): nothing when the plan
    leaves it alone, fhe_mul_const on the n_out rows that are left when no ModReduce is in it, else ONE fhe_mod_reduce_multi_limbs_pair.
    qs: the moduli of the tower's rows (default: those of its context limbs).  Returns the two Towers (the inputs when untouched)."""
    if plan.untouched():
        return c0, c1
    sizeQl = c0.n_limbs
    if qs is None:
        qs = ctx.q[:sizeQl] if c0.limb_idx is None else ctx.q[c0.limb_idx]
    qs = [int(v) for v in qs]
    kept = None if c0.limb_idx is None else c0.limb_idx[:plan.n_out]
    if not plan.drop_rows:
        consts = np.array([plan.scalar % q for q in qs[:plan.n_out]], np.uint64)
        o0, o1 = ctx.empty(1, plan.n_out, kept, c0.fmt), ctx.empty(1, plan.n_out, kept, c0.fmt)
        ctx.lib.check(ctx.lib.L.fhe_mul_const_pair(ctx.h, o0.ptr, o1.ptr, c0.ptr, c1.ptr, consts.ctypes.data_as(u64p),
                                                   None if kept is None else kept.ctypes.data_as(u32p), plan.n_out, stream))
        ctx.sync(stream)
        return o0, o1
    negt, inv = mod_reduce_multi_tables(qs, t, plan.drop_rows)
    return mod_reduce_multi_pair(ctx, c0, c1, t, negt, inv, scalar=plan.scalar, drop_rows=plan.drop_rows, n_out=plan.n_out, stream=stream)


def mod_reduce_chain(ctx, x, levels, t, stream=None):
    """`levels` consecutive DCRTPoly::ModReduce calls (dcrtpoly-impl.h:736-755) on a COEFFICIENT Tower, its last limb first, in one
    launch per 16 levels (fhe_mod_reduce_chain): what the COEFFICIENT branch of PKEBGVRNS::Decrypt runs on every element."""
    sizeQl = x.n_limbs
    need = ctx.lib.L.fhe_mod_reduce_chain_workspace_bytes(ctx.h, sizeQl, levels, x.batch)
    ws = ctx.malloc(need) if need else None
    kept = None if x.limb_idx is None else x.limb_idx[:max(sizeQl - levels, 1)]
    out = ctx.empty(x.batch, max(sizeQl - levels, 1), kept, COEFFICIENT)
    try:
        ctx.lib.check(ctx.lib.L.fhe_mod_reduce_chain(ctx.h, x.ptr, x._li(), sizeQl, levels, t, x.batch, out.ptr, ws, need, stream))
        ctx.sync(stream)
    finally:
        if ws:
            ctx.free(ws)
    return out


def mod_reduce_to_t(ctx, x, t, stream=None):
    """the ModReduce chain of a COEFFICIENT Tower down to one limb and DecryptionCRTInterpolate(t) of it (fhe_mod_reduce_to_t): the tail of
    PKEBGVRNS::Decrypt and MultipartyDecryptFusion; returns uint64 [batch][N] in [0, t)"""
    sizeQl = x.n_limbs
    need = ctx.lib.L.fhe_mod_reduce_chain_workspace_bytes(ctx.h, sizeQl, sizeQl - 1, x.batch)
    ws = ctx.malloc(need) if need else None
    d = ctx.malloc(x.batch * ctx.N * 8)
    try:
        ctx.lib.check(ctx.lib.L.fhe_mod_reduce_to_t(ctx.h, x.ptr, x._li(), sizeQl, t, x.batch, d, ws, need, stream))
        return ctx.download(d, (x.batch, ctx.N), stream)
    finally:
        ctx.free(d)
        if ws:
            ctx.free(ws)


def bgv_decrypt(ctx, elements, s, t, stream=None):
    """PKEBGVRNS::Decrypt on EVALUATION ciphertexts (bgvrns-pke.cpp:52-60, 96) through fhe_bgv_decrypt: elements = 2 or 3 Towers
    [batch][sizeQl][N], s = the secret key, one Tower [1][sizeQl][N] over the same limbs; returns the NativePoly words, uint64 [batch][N]"""
    c0 = elements[0]
    need = ctx.lib.L.fhe_bgv_decrypt_workspace_bytes(ctx.h, len(elements), c0.n_limbs, c0.batch)
    ws = ctx.malloc(max(need, 8))
    d = ctx.malloc(c0.batch * ctx.N * 8)
    ptrs = (vp * len(elements))(*[e.ptr.value if hasattr(e.ptr, "value") else e.ptr for e in elements])
    try:
        ctx.lib.check(ctx.lib.L.fhe_bgv_decrypt(ctx.h, ptrs, len(elements), s.ptr, c0._li(), c0.n_limbs, t, c0.batch, d, ws, need, stream))
        return ctx.download(d, (c0.batch, ctx.N), stream)
    finally:
        ctx.free(d)
        ctx.free(ws)


def _elem_ptrs(elements):
    """C array of the elements' device pointers (NULL for None)"""
    return (vp * len(elements))(*[None if e is None else e.ptr.value if hasattr(e.ptr, "value") else e.ptr for e in elements])


def decrypt_chunk(ctx, n_limbs, batch):
    """ciphertexts a workgroup of the decrypt combine walks (fhe_decrypt_chunk)"""
    return ctx.lib.L.fhe_decrypt_chunk(ctx.h, n_limbs, batch)


def decrypt_core(ctx, elements, s, noise=None, ns=1, with_c0=True, out_format=EVALUATION, out=None, stream=None):
    """PKERNS::DecryptCore (rns-pke.cpp:199-225) through fhe_decrypt_core: elements = 2 to 4 EVALUATION Towers [batch][nLimbs][N]
    (elements[0] may be None with with_c0=False: MultipartyDecryptMain), s [1][>= nLimbs][N] (its first nLimbs rows are used), noise a
    Tower like the elements or None.  Returns b in out_format: a new Tower, or `out` (which may be elements[0] or noise)."""
    c1 = elements[1]
    assert s.n_limbs >= c1.n_limbs
    b = c1.like() if out is None else out
    ctx.lib.check(ctx.lib.L.fhe_decrypt_core(ctx.h, _elem_ptrs(elements), len(elements), s.ptr, c1._li(), c1.n_limbs, c1.batch,
                                             None if noise is None else noise.ptr, ns, 1 if with_c0 else 0, out_format, b.ptr, stream))
    b.fmt = out_format
    return b


def ckks_decrypt(ctx, elements, s, noise=None, stream=None):
    """PKECKKSRNS::Decrypt up to the interpolation (ckksrns-pke.cpp:44-96): the COEFFICIENT tower of b as uint64 [batch][nLimbs][N] on the
    host (one limb: the NativePoly; more: what CRTInterpolate takes).  noise: the flooding term of NOISE_FLOODING_DECRYPT, EVALUATION."""
    return decrypt_core(ctx, elements, s, noise=noise, out_format=COEFFICIENT, stream=stream).to_host()


class BfvDecrypt:
    """PKEBFVRNS::Decrypt at sizeQl == sizeQ (bfvrns-pke.cpp:215-245) with tables derived from the moduli and t (fhe_bfv_decrypt_create)."""

    BEHZ, HPS, HPSPOVERQ, HPSPOVERQLEVELED = 0, 1, 2, 3
    TABLES = ("tQHatInvModqDivqModt", "tQHatInvModqBDivqModt", "tQHatInvModqDivqFrac", "tQHatInvModqBDivqFrac", "tgamma",
              "tgammaQHatInvModq", "negInvqModtgamma")

    def __init__(self, ctx, t, technique=HPS, limb_idx=None, size_q=None):
        self.ctx, self.t, self.technique = ctx, t, technique
        self.limb_idx = None if limb_idx is None else np.ascontiguousarray(np.asarray(limb_idx, dtype=np.uint32))
        self.sizeQ = (ctx.L if size_q is None else size_q) if limb_idx is None else len(self.limb_idx)
        h = vp()
        ctx.lib.check(ctx.lib.L.fhe_bfv_decrypt_create(ctx.h, None if limb_idx is None else self.limb_idx.ctypes.data_as(u32p), self.sizeQ,
                                                       t, technique, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.L.fhe_bfv_decrypt_destroy(self.h)
            self.h = None

    def table(self, name):
        """a derived table as a flat uint64 array (the Frac tables as bit patterns: .view(np.float64)); None if the plan has none"""
        tid = self.TABLES.index(name) if isinstance(name, str) else int(name)
        n = self.ctx.lib.L.fhe_bfv_decrypt_table(self.h, tid, None, 0)
        if n == 0:
            return None
        out = np.zeros(n, np.uint64)
        self.ctx.lib.L.fhe_bfv_decrypt_table(self.h, tid, out.ctypes.data_as(u64p), n)
        return out

    def workspace_bytes(self, batch):
        return self.ctx.lib.L.fhe_bfv_decrypt_workspace_bytes(self.h, batch)

    def _run(self, batch, call, stream):
        ctx, need = self.ctx, self.workspace_bytes(batch)
        ws, d = ctx.malloc(max(need, 8)), ctx.malloc(batch * ctx.N * 8)
        try:
            ctx.lib.check(call(d, ws, need))
            return ctx.download(d, (batch, ctx.N), stream)
        finally:
            ctx.free(d)
            ctx.free(ws)

    def Decrypt(self, elements, s, stream=None):
        """elements: 2 to 4 EVALUATION Towers [batch][sizeQ][N], s the secret key [1][sizeQ][N]; returns the NativePoly words modulo t,
        uint64 [batch][N]"""
        L, batch = self.ctx.lib.L, elements[0].batch
        return self._run(batch, lambda d, ws, need: L.fhe_bfv_decrypt(self.h, _elem_ptrs(elements), len(elements), s.ptr, batch, d, ws,
                                                                      need, stream), stream)

    def DecryptB(self, b, stream=None):
        """the tail alone on a Tower b [batch][sizeQ][N] in either format (MultipartyDecryptFusion after its sum); b is only read"""
        L = self.ctx.lib.L
        return self._run(b.batch, lambda d, ws, need: L.fhe_bfv_decrypt_b(self.h, b.ptr, 1 if b.fmt == EVALUATION else 0, b.batch, d, ws,
                                                                          need, stream), stream)


def scale_and_round_native(ctx, x, t, tab_modt, frac, tab_bmodt=None, bfrac=None, stream=None):
    """DCRTPoly::ScaleAndRound -> NativePoly mod t (BFV decryption, dcrtpoly-impl.h:1190-1467); returns uint64 [batch][N]"""
    ta = np.ascontiguousarray(tab_modt, dtype=np.uint64)
    fr = np.ascontiguousarray(frac, dtype=np.float64)
    tb = np.ascontiguousarray(tab_bmodt, dtype=np.uint64) if tab_bmodt is not None else None
    bf = np.ascontiguousarray(bfrac, dtype=np.float64) if bfrac is not None else None
    out = ctx.malloc(x.batch * ctx.N * 8)
    li = x.limb_idx.ctypes.data_as(u32p) if x.limb_idx is not None else None
    f64p = C.POINTER(C.c_double)
    ctx.lib.check(ctx.lib.L.fhe_scale_and_round_native(ctx.h, x.ptr, li, x.n_limbs, t, ta.ctypes.data_as(u64p),
                                                       tb.ctypes.data_as(u64p) if tb is not None else None,
                                                       fr.ctypes.data_as(f64p), bf.ctypes.data_as(f64p) if bf is not None else None,
                                                       x.batch, out, stream))
    host = np.empty((x.batch, ctx.N), np.uint64)
    ctx.lib.check(ctx.lib.L.fhe_memcpy_d2h(ctx.h, host.ctypes.data_as(vp), out, host.nbytes, stream))
    ctx.sync(stream)
    ctx.free(out)
    return host


def scale_and_round_behz_decrypt(ctx, x, tgamma, tgamma_qhat_modq, neg_invq_mod_tgamma, stream=None):
    """DCRTPoly::ScaleAndRound, BEHZ decryption overload (dcrtpoly-impl.h:1631-1671); returns uint64 [batch][N]"""
    ta = np.ascontiguousarray(tgamma_qhat_modq, dtype=np.uint64)
    tb = np.ascontiguousarray(neg_invq_mod_tgamma, dtype=np.uint64)
    out = ctx.malloc(x.batch * ctx.N * 8)
    li = x.limb_idx.ctypes.data_as(u32p) if x.limb_idx is not None else None
    ctx.lib.check(ctx.lib.L.fhe_scale_and_round_behz_decrypt(ctx.h, x.ptr, li, x.n_limbs, tgamma, ta.ctypes.data_as(u64p),
                                                             tb.ctypes.data_as(u64p), x.batch, out, stream))
    host = np.empty((x.batch, ctx.N), np.uint64)
    ctx.lib.check(ctx.lib.L.fhe_memcpy_d2h(ctx.h, host.ctypes.data_as(vp), out, host.nbytes, stream))
    ctx.sync(stream)
    ctx.free(out)
    return host


class ScaleAndRoundPlan:
    """DCRTPoly::ScaleAndRound / ApproxScaleAndRound with the reference's tables (dcrtpoly-impl.h:1470-1628)."""

    def __init__(self, ctx, sizeI, out_idx, tab, frac=None):
        self.ctx, self.sizeI = ctx, sizeI
        self.out_idx = np.ascontiguousarray(np.asarray(out_idx, dtype=np.uint32))
        tab = np.ascontiguousarray(tab, dtype=np.uint64)
        assert tab.shape == (len(self.out_idx), sizeI + 1)
        fp = None
        if frac is not None:
            frac = np.ascontiguousarray(frac, dtype=np.float64)
            fp = frac.ctypes.data_as(C.POINTER(C.c_double))
        h = vp()
        ctx.lib.check(ctx.lib.L.fhe_sr_plan_create(ctx.h, sizeI, self.out_idx.ctypes.data_as(u32p), len(self.out_idx),
                                                   tab.ctypes.data_as(u64p), fp, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.L.fhe_sr_plan_destroy(self.h)
            self.h = None

    def run(self, x, output_first, stream=None):
        out = self.ctx.empty(x.batch, len(self.out_idx), self.out_idx, COEFFICIENT)
        self.ctx.lib.check(self.ctx.lib.L.fhe_scale_and_round(self.h, x.ptr, 1 if output_first else 0, out.ptr, x.batch, stream))
        return out


def scale_and_round_p_over_q(ctx, x, limb_idx, stream=None):
    """DCRTPoly::ScaleAndRoundPOverQ (dcrtpoly-impl.h:1674-1689): x over limb_idx (sizeQ+1 limbs) -> sizeQ limbs"""
    li = np.ascontiguousarray(np.asarray(limb_idx, dtype=np.uint32))
    sizeQ = len(li) - 1
    out = ctx.empty(x.batch, sizeQ, li[:sizeQ], COEFFICIENT)
    ctx.lib.check(ctx.lib.L.fhe_scale_and_round_p_over_q(ctx.h, x.ptr, li.ctypes.data_as(u32p), sizeQ, out.ptr, x.batch, stream))
    return out


class Behz:
    """BEHZ base conversions over a context that holds the Q limbs and the Bsk limbs."""

    def __init__(self, ctx, q_idx, bsk_idx, t):
        self.ctx = ctx
        self.q_idx = np.ascontiguousarray(np.asarray(q_idx, dtype=np.uint32))
        self.bsk_idx = np.ascontiguousarray(np.asarray(bsk_idx, dtype=np.uint32))
        self.numQ, self.numBsk = len(self.q_idx), len(self.bsk_idx)
        h = vp()
        ctx.lib.check(ctx.lib.L.fhe_behz_create(ctx.h, self.q_idx.ctypes.data_as(u32p), self.numQ,
                                                self.bsk_idx.ctypes.data_as(u32p), t, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.L.fhe_behz_destroy(self.h)
            self.h = None

    def FastBaseConvqToBskMontgomery(self, xq_host, eval_format, stream=None):
        """xq_host: uint64 [batch][numQ][N]; returns the extended tower [batch][numQ+numBsk][N] (EVALUATION)"""
        xq_host = np.asarray(xq_host, dtype=np.uint64)
        B, N = xq_host.shape[0], self.ctx.N
        full = np.zeros((B, self.numQ + self.numBsk, N), np.uint64)
        full[:, :self.numQ] = xq_host
        t = self.ctx.tower(full, limb_idx=np.concatenate([self.q_idx, self.bsk_idx]))
        wsb = self.ctx.lib.L.fhe_behz_workspace_bytes(self.h, B)
        ws = self.ctx.malloc(wsb)
        self.ctx.lib.check(self.ctx.lib.L.fhe_behz_q_to_bsk(self.h, t.ptr, 1 if eval_format else 0, B, ws, wsb, stream))
        self.ctx.sync(stream)
        self.ctx.free(ws)
        t.fmt = EVALUATION
        return t

    def FastRNSFloorq(self, t, stream=None):
        self.ctx.lib.check(self.ctx.lib.L.fhe_behz_floorq(self.h, t.ptr, t.batch, stream))
        return t

    def FastBaseConvSK(self, t, stream=None):
        out = self.ctx.empty(t.batch, self.numQ, self.q_idx, COEFFICIENT)
        self.ctx.lib.check(self.ctx.lib.L.fhe_behz_conv_sk(self.h, t.ptr, out.ptr, t.batch, stream))
        return out

    def EvalMult(self, ks_plan, a0, a1, b0, b1, stream=None):
        """LeveledSHEBase::EvalMult(ct, ct, key) on BFV/BEHZ ciphertexts: EvalMultNoRelin + relinearisation with the
        key-switch plan's evaluation key; returns (c0, c1), EVALUATION"""
        B = a0.batch
        c0, c1 = (self.ctx.empty(B, self.numQ, self.q_idx, EVALUATION) for _ in range(2))
        L = self.ctx.lib.L
        wsb = L.fhe_bfv_eval_mult_relin_workspace_bytes(self.h, ks_plan.h, B)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_bfv_eval_mult_relin_behz(self.h, ks_plan.h, ks_plan.key, a0.ptr, a1.ptr, b0.ptr, b1.ptr,
                                                              c0.ptr, c1.ptr, B, ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return c0, c1

    def EvalMultNoRelin(self, a0, a1, b0, b1, out_eval=False, stream=None):
        """LeveledSHEBFVRNS::EvalMult (BEHZ) on device towers [batch][numQ][N] (EVALUATION); returns (d0, d1, d2)"""
        B = a0.batch
        fmt = EVALUATION if out_eval else COEFFICIENT
        d = [self.ctx.empty(B, self.numQ, self.q_idx, fmt) for _ in range(3)]
        L = self.ctx.lib.L
        wsb = L.fhe_bfv_eval_mult_behz_workspace_bytes(self.h, B)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_bfv_eval_mult_behz(self.h, a0.ptr, a1.ptr, b0.ptr, b1.ptr, d[0].ptr, d[1].ptr,
                                                        d[2].ptr, 1 if out_eval else 0, B, ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return d


HPS, HPSPOVERQ, HPSPOVERQLEVELED = 1, 2, 3  # MultiplicationTechnique (constants-defs.h:97)


class Hps:
    """BFV EvalMult of the HPS family over a context that holds the Q limbs and the R limbs (Lib.hps_r)."""

    # fhe_hps_table ids
    TABLES = ("QlHatInvModq", "QlHatModr", "alphaQlModr", "qInv", "RlHatInvModr", "RlHatModq", "alphaRlModq", "rInv",
              "tRSHatInvModsDivsModr", "tRSHatInvModsDivsFrac", "tQlSlHatInvModsDivsModq", "tQlSlHatInvModsDivsFrac",
              "negRlQHatInvModq", "negRlQlHatInvModq", "qInvModr", "QlQHatInvModqDivqModq", "QlQHatInvModqDivqFrac", "QlHatModq")

    def __init__(self, ctx, q_idx, r_idx, t, technique):
        self.ctx = ctx
        self.q_idx = np.ascontiguousarray(np.asarray(q_idx, dtype=np.uint32))
        self.r_idx = np.ascontiguousarray(np.asarray(r_idx, dtype=np.uint32))
        self.numQ, self.numR, self.technique = len(self.q_idx), len(self.r_idx), technique
        h = vp()
        ctx.lib.check(ctx.lib.L.fhe_hps_create(ctx.h, self.q_idx.ctypes.data_as(u32p), self.numQ, self.r_idx.ctypes.data_as(u32p),
                                               self.numR, t, technique, C.byref(h)))
        self.h = h
        self._ws = None  # rotations and relinearisation on a BV key: the digits of the last FastRotationPrecompute stay here (hoisting)
        self._ws_bytes = 0

    def close(self):
        if self.h:
            self.ctx.lib.L.fhe_hps_destroy(self.h)
            self.h = None
        if self._ws is not None and self.ctx.h:
            self.ctx.free(self._ws)
        self._ws = None

    def table(self, name, level=0):
        """a derived table as a flat uint64 array (doubles as their bit patterns: .view(np.float64)); None if absent"""
        tid = self.TABLES.index(name) if isinstance(name, str) else int(name)
        n = self.ctx.lib.L.fhe_hps_table(self.h, tid, level, None, 0)
        if n == 0:
            return None
        out = np.zeros(n, np.uint64)
        self.ctx.lib.L.fhe_hps_table(self.h, tid, level, out.ctypes.data_as(u64p), n)
        return out

    def workspace_bytes(self, size_ql, batch):
        return self.ctx.lib.L.fhe_bfv_eval_mult_hps_workspace_bytes(self.h, size_ql, batch)

    def EvalMultNoRelin(self, a0, a1, b0, b1, size_ql=None, out_eval=False, stream=None):
        """LeveledSHEBFVRNS::EvalMult (HPS / HPSPOVERQ / HPSPOVERQLEVELED) on device towers [batch][numQ][N] (EVALUATION);
        size_ql = numQ - levelsDropped (HPSPOVERQLEVELED only; default numQ); returns (d0, d1, d2)"""
        B = a0.batch
        size_ql = self.numQ if size_ql is None else size_ql
        fmt = EVALUATION if out_eval else COEFFICIENT
        d = [self.ctx.empty(B, self.numQ, self.q_idx, fmt) for _ in range(3)]
        L = self.ctx.lib.L
        wsb = max(L.fhe_bfv_eval_mult_hps_workspace_bytes(self.h, size_ql, B), 8)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_bfv_eval_mult_hps(self.h, a0.ptr, a1.ptr, b0.ptr, b1.ptr, d[0].ptr, d[1].ptr, d[2].ptr,
                                                       size_ql, 1 if out_eval else 0, B, ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return d

    def bv_workspace(self, size_ql, base_bits, batch):
        need = self.ctx.lib.L.fhe_bfv_bv_workspace_bytes(self.h, size_ql, base_bits, batch)
        if need > self._ws_bytes:
            if self._ws is not None:
                self.ctx.free(self._ws)
            self._ws = self.ctx.malloc(need)
            self._ws_bytes = need
        return self._ws, self._ws_bytes

    def FastRotationPrecompute(self, c1, base_bits, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:782-813
        """the digits of c1 (EVALUATION) at size_ql = numQ - levelsDropped limbs, left at the start of the plan's workspace"""
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.bv_workspace(size_ql, base_bits, c1.batch)
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_fast_rotation_precompute_bv(self.h, c1.ptr, size_ql, base_bits, c1.batch, ws, wsb, stream))
        return ws, wsb

    def FastRotation(self, bv_key, c0, k, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:815-882
        """on the digits of the last FastRotationPrecompute (same size_ql, the key's base_bits); k = automorphism index"""
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.bv_workspace(size_ql, bv_key.base_bits, c0.batch)
        o0, o1 = c0.like(), c0.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_eval_fast_rotation_bv(self.h, bv_key.h, c0.ptr, k, size_ql, c0.batch, o0.ptr, o1.ptr, ws, wsb,
                                                                        stream))
        return o0, o1

    def Automorphism(self, bv_key, c0, c1, k, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:767-780
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.bv_workspace(size_ql, bv_key.base_bits, c0.batch)
        o0, o1 = c0.like(), c0.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_eval_automorphism_bv(self.h, bv_key.h, c0.ptr, c1.ptr, k, size_ql, c0.batch, o0.ptr, o1.ptr,
                                                                       ws, wsb, stream))
        return o0, o1

    def Relinearize(self, bv_key, d0, d1, d2, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:888-938
        """(d0 + Expand(ks0(d2)), d1 + Expand(ks1(d2))), EVALUATION; the three inputs share one format (COEFFICIENT as EvalMultNoRelin
        leaves them, or EVALUATION)"""
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.bv_workspace(size_ql, bv_key.base_bits, d0.batch)
        c0, c1 = (self.ctx.empty(d0.batch, self.numQ, self.q_idx, EVALUATION) for _ in range(2))
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_relinearize_bv(self.h, bv_key.h, d0.ptr, d1.ptr, d2.ptr, 1 if d2.fmt == EVALUATION else 0,
                                                                 size_ql, d0.batch, c0.ptr, c1.ptr, ws, wsb, stream))
        return c0, c1

    def EvalMult(self, bv_key, a0, a1, b0, b1, size_ql=None, size_ql_relin=None, stream=None):
        """LeveledSHEBase::EvalMult(ct, ct, key) with a BV key (base-leveledshe.cpp:201-214): the product above, then KeySwitchCore on its
        third element at numQ limbs added to the first two; returns (c0, c1), EVALUATION.  size_ql_relin given: LeveledSHEBFVRNS::EvalMult
        (bfvrns-leveledshe.cpp:735-741) with the relinearisation at size_ql_relin = numQ - levelsDropped(key switch) limbs"""
        B = a0.batch
        size_ql = self.numQ if size_ql is None else size_ql
        c0, c1 = (self.ctx.empty(B, self.numQ, self.q_idx, EVALUATION) for _ in range(2))
        L = self.ctx.lib.L
        if size_ql_relin is not None:
            wsb = max(L.fhe_bfv_eval_mult_relin_hps_bv_leveled_workspace_bytes(self.h, size_ql, size_ql_relin, bv_key.base_bits, B), 8)
            ws = self.ctx.malloc(wsb)
            try:
                self.ctx.lib.check(L.fhe_bfv_eval_mult_relin_hps_bv_leveled(self.h, bv_key.h, a0.ptr, a1.ptr, b0.ptr, b1.ptr, c0.ptr, c1.ptr,
                                                                            size_ql, size_ql_relin, B, ws, wsb, stream))
                self.ctx.sync(stream)
            finally:
                self.ctx.free(ws)
            return c0, c1
        wsb = max(L.fhe_bfv_eval_mult_relin_hps_bv_workspace_bytes(self.h, size_ql, bv_key.base_bits, B), 8)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_bfv_eval_mult_relin_hps_bv(self.h, bv_key.h, a0.ptr, a1.ptr, b0.ptr, b1.ptr, c0.ptr, c1.ptr, size_ql, B,
                                                                ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return c0, c1


class BfvHybrid:
    """BFV of the HPS family on HYBRID keys: an Hps plan paired with a KeySwitchPlan of the same context (Q the context's leading limbs, the
    plan's sizeQ == numQ).  Keys are KeySwitchPlan handles (make_key / upload_key).  size_ql = numQ - levelsDropped for the KEY SWITCH: 1 ...
    numQ for HPSPOVERQLEVELED, numQ otherwise; None = numQ."""

    def __init__(self, hps, ks_plan):
        self.ctx, self.hps, self.ks = hps.ctx, hps, ks_plan
        self.numQ, self.q_idx = hps.numQ, hps.q_idx
        h = vp()
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_hybrid_create(hps.h, ks_plan.h, C.byref(h)))
        self.h = h
        self._ws = None  # the digits of the last FastRotationPrecompute stay here (hoisting)
        self._ws_bytes = 0

    def close(self):
        if self.h:
            self.ctx.lib.L.fhe_bfv_hybrid_destroy(self.h)
            self.h = None
        if self._ws is not None and self.ctx.h:
            self.ctx.free(self._ws)
        self._ws = None

    def workspace(self, size_ql, batch):
        need = self.ctx.lib.L.fhe_bfv_hybrid_workspace_bytes(self.h, size_ql, batch)
        if need > self._ws_bytes:
            if self._ws is not None:
                self.ctx.free(self._ws)
            self._ws = self.ctx.malloc(need)
            self._ws_bytes = need
        return self._ws, self._ws_bytes

    def FastRotationPrecompute(self, c1, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:782-813
        """the digits of c1 (EVALUATION) at size_ql limbs, left in the plan's workspace"""
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.workspace(size_ql, c1.batch)
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_fast_rotation_precompute_hybrid(self.h, c1.ptr, size_ql, c1.batch, ws, wsb, stream))
        return ws, wsb

    def FastRotation(self, key, c0, c1, k, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:815-882
        """on the digits of the last FastRotationPrecompute(c1) at the same size_ql; k = automorphism index"""
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.workspace(size_ql, c0.batch)
        o0, o1 = c0.like(), c0.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_eval_fast_rotation_hybrid(self.h, key, c0.ptr, c1.ptr, k, size_ql, c0.batch, o0.ptr, o1.ptr,
                                                                            ws, wsb, stream))
        return o0, o1

    def Automorphism(self, key, c0, c1, k, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:767-780
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.workspace(size_ql, c0.batch)
        o0, o1 = c0.like(), c0.like()
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_eval_automorphism_hybrid(self.h, key, c0.ptr, c1.ptr, k, size_ql, c0.batch, o0.ptr, o1.ptr,
                                                                           ws, wsb, stream))
        return o0, o1

    def Relinearize(self, key, d0, d1, d2, size_ql=None, stream=None):  # bfvrns-leveledshe.cpp:888-938
        """(d0 + Expand(ks0(d2)), d1 + Expand(ks1(d2))), EVALUATION; the three inputs share one format (COEFFICIENT as EvalMultNoRelin
        leaves them, or EVALUATION)"""
        size_ql = self.numQ if size_ql is None else size_ql
        ws, wsb = self.workspace(size_ql, d0.batch)
        c0, c1 = (self.ctx.empty(d0.batch, self.numQ, self.q_idx, EVALUATION) for _ in range(2))
        self.ctx.lib.check(self.ctx.lib.L.fhe_bfv_relinearize_hybrid(self.h, key, d0.ptr, d1.ptr, d2.ptr, 1 if d2.fmt == EVALUATION else 0,
                                                                     size_ql, d0.batch, c0.ptr, c1.ptr, ws, wsb, stream))
        return c0, c1

    def EvalMult(self, key, a0, a1, b0, b1, size_ql=None, size_ql_relin=None, stream=None):  # bfvrns-leveledshe.cpp:735-741
        """LeveledSHEBFVRNS::EvalMult(ct, ct, key): the product at size_ql limbs, the relinearisation at size_ql_relin; returns (c0, c1),
        EVALUATION"""
        B = a0.batch
        size_ql = self.numQ if size_ql is None else size_ql
        size_ql_relin = self.numQ if size_ql_relin is None else size_ql_relin
        c0, c1 = (self.ctx.empty(B, self.numQ, self.q_idx, EVALUATION) for _ in range(2))
        L = self.ctx.lib.L
        wsb = max(L.fhe_bfv_eval_mult_relin_hps_hybrid_workspace_bytes(self.h, size_ql, size_ql_relin, B), 8)
        ws = self.ctx.malloc(wsb)
        try:
            self.ctx.lib.check(L.fhe_bfv_eval_mult_relin_hps_hybrid(self.h, key, a0.ptr, a1.ptr, b0.ptr, b1.ptr, c0.ptr, c1.ptr, size_ql,
                                                                    size_ql_relin, B, ws, wsb, stream))
            self.ctx.sync(stream)
        finally:
            self.ctx.free(ws)
        return c0, c1
