"""seal-embedded_amd: Python (ctypes) binding of libseal_embedded_amd.so.

This is plumbing for tests and bench.py: PyTorch supplies device memory and streams, every
compute call goes straight through the C ABI declared in include/seal_embedded_amd.h.
There is no Python or CPU implementation of the path here -- if the HIP library is missing or
no GPU is present, construction fails loudly.

The directory name contains a hyphen, so load it through `__graft_entry__.load_package()` (or
importlib) under the module name `seal_embedded_amd`.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libseal_embedded_amd.so")
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include", "seal_embedded_amd.h")

STAGES = ("cbd", "uniform", "ternary", "encode_encrypt", "encode_rns", "ntt_fuse")

SE_SUCCESS = 0


class SealEmbeddedAmdError(RuntimeError):
    pass


TESTHOOKS_LIB_DIR = os.path.join(HERE, "lib", "testhooks")   # the -DSEAMD_TEST_HOOKS build (tests only)


def build_library(jobs=8, verbose=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU), and beside it the
    test build (se_api.cpp under -DSEAMD_TEST_HOOKS: fault injection) the GPU tests link against."""
    cmd = ["make", "-C", CSRC, f"-j{jobs}", "all", "testhooks"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None

# every symbol include/seal_embedded_amd.h declares (checked by tests/test_cabi.py)
EXPORTED_SYMBOLS = (
    "se_setup_custom", "se_setup", "se_setup_default", "se_encrypt_seeded", "se_encrypt",
    "se_cleanup", "se_encrypt_batch",
    "se_amd_create", "se_amd_destroy", "se_amd_degree", "se_amd_nprimes", "se_amd_scale",
    "se_amd_moduli", "se_amd_index_map", "se_amd_set_secret_key", "se_amd_set_public_key",
    "se_amd_load_keys_from_dir", "se_amd_gen_public_key", "se_amd_gen_keys_batch", "se_amd_encrypt_sym_device", "se_amd_encrypt_asym_device", "se_amd_encrypt_sym_seeded_device",
    "se_amd_expand_c1_device",
    "se_amd_encode_ntt_device", "se_amd_encrypt_sym_host", "se_amd_encrypt_asym_host",
    "se_amd_encode_device", "se_amd_ntt_device", "se_amd_intt_device", "se_amd_decrypt_decode_device", "se_amd_prng_blocks_device",
    "se_amd_sample_uniform_device", "se_amd_sample_ternary_device", "se_amd_sample_cbd_device",
    "se_amd_pack_ternary_host", "se_amd_word_ops_device", "se_amd_pack_seal_ciphertext_host", "se_amd_format_poly_text",
    "se_amd_format_values_text", "se_amd_write_ciphertext_text", "se_amd_save_secret_key_file",
    "se_amd_save_public_key_files", "se_amd_set_profiling", "se_amd_stage_ms",
    "se_amd_group_create", "se_amd_group_destroy", "se_amd_group_size", "se_amd_group_ctx", "se_amd_group_device",
    "se_amd_group_partition", "se_amd_group_set_secret_key", "se_amd_group_set_public_key", "se_amd_group_reserve",
    "se_amd_encrypt_sym_multi_device", "se_amd_encrypt_asym_multi_device", "se_amd_encode_ntt_multi_device",
    "se_amd_set_reject_list_capacity", "se_amd_set_speculation_capacity", "se_amd_set_host_chunk", "se_amd_host_tables", "se_amd_ifft_table_sha256", "se_amd_reserve", "se_amd_set_debug_flags", "se_amd_set_pipeline", "se_amd_set_asym_chunks", "se_amd_last_error", "se_amd_version",
    "se_amd_set_secret_keyring", "se_amd_set_public_keyring", "se_amd_encrypt_sym_keyed_device",
    "se_amd_encrypt_asym_keyed_device", "se_amd_decrypt_decode_keyed_device",
    "se_amd_decrypt_full_device", "se_amd_decrypt_full_keyed_device", "se_amd_crt_constants",
    "se_amd_ct_lincomb_device", "se_amd_set_lincomb_split",
    "se_amd_ct_rescale_device", "se_amd_ct_mul_plain_device", "se_amd_decrypt_level_device",
    "se_amd_decrypt_level_keyed_device", "se_amd_rescale_constants",
    "se_amd_ct_mul_device", "se_amd_decrypt3_level_device", "se_amd_decrypt3_level_keyed_device",
    "se_amd_gen_relin_key", "se_amd_set_relin_key", "se_amd_ct_relin_device",
    "se_amd_galois_element", "se_amd_galois_table", "se_amd_gen_galois_keys", "se_amd_set_galois_keys",
    "se_amd_ct_galois_device", "se_amd_ct_galois_many_device", "se_amd_ct_galois_sum_device",
    "se_amd_lintrans_create", "se_amd_lintrans_destroy", "se_amd_ct_lintrans_device",
    "se_amd_gen_relin_key_sp", "se_amd_set_relin_key_sp", "se_amd_gen_galois_keys_sp", "se_amd_set_galois_keys_sp",
    "se_amd_ct_relin_sp_device", "se_amd_ct_galois_sp_device", "se_amd_ct_drop_primes_device",
    "se_amd_ct_galois_sum_sp_device", "se_amd_lintrans_create_sp", "se_amd_ct_lintrans_sp_device",
    "se_amd_ct_mul_plain_sum_device", "se_amd_ct_galois_accum_device", "se_amd_bsgs_create", "se_amd_bsgs_destroy",
    "se_amd_bsgs_workspace_bytes", "se_amd_ct_bsgs_device",
    "se_amd_ct_galois_many_ext_sp_device", "se_amd_ct_mul_plain_sum_ext_sp_device", "se_amd_ct_mod_down_sp_device",
    "se_amd_ct_galois_accum_sp_device", "se_amd_bsgs_create_sp", "se_amd_ct_bsgs_sp_device",
    "se_amd_gen_switch_keys_sp", "se_amd_set_switch_keyring_sp", "se_amd_ct_switch_keyed_sp_device",
    "se_amd_ct_switch_sum_keyed_sp_device",
    "se_amd_ct_mul_sum_device", "se_amd_ct_dot_sp_device",
    "se_amd_ct_pack_sp_device",
    "se_amd_ct_affine_rescale_device", "se_amd_poly_create", "se_amd_poly_destroy", "se_amd_poly_terms",
    "se_amd_poly_result", "se_amd_poly_workspace_bytes", "se_amd_ct_poly_sp_device",
)


def lib():
    """Load the shared library (never builds implicitly; never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SealEmbeddedAmdError(
            f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    L.se_amd_last_error.restype = C.c_char_p
    L.se_amd_version.restype = C.c_char_p
    L.se_amd_create.argtypes = [C.POINTER(vp), sz, sz, i32]
    L.se_amd_destroy.argtypes = [vp]
    L.se_amd_destroy.restype = None
    L.se_amd_degree.argtypes = [vp]
    L.se_amd_degree.restype = sz
    L.se_amd_nprimes.argtypes = [vp]
    L.se_amd_nprimes.restype = sz
    L.se_amd_scale.argtypes = [vp]
    L.se_amd_scale.restype = C.c_double
    L.se_amd_moduli.argtypes = [vp, vp]
    L.se_amd_index_map.argtypes = [vp, vp]
    L.se_amd_set_secret_key.argtypes = [vp, vp]
    L.se_amd_set_public_key.argtypes = [vp, vp, vp]
    L.se_amd_load_keys_from_dir.argtypes = [vp, C.c_char_p, i32]
    L.se_amd_gen_public_key.argtypes = [vp, vp, vp, vp, vp, vp]
    L.se_amd_gen_keys_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_encrypt_sym_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_encrypt_asym_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_encrypt_sym_seeded_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    L.se_amd_expand_c1_device.argtypes = [vp, vp, sz, vp, vp]
    L.se_amd_encode_ntt_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.se_amd_encrypt_sym_host.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_encrypt_asym_host.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp]
    L.se_amd_encode_device.argtypes = [vp, vp, sz, vp, vp, vp]
    L.se_amd_ntt_device.argtypes = [vp, sz, vp, sz, vp]
    L.se_amd_intt_device.argtypes = [vp, sz, vp, sz, vp]
    L.se_amd_decrypt_decode_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
    L.se_amd_prng_blocks_device.argtypes = [vp, vp, vp, vp, sz, sz, vp]
    L.se_amd_sample_uniform_device.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    L.se_amd_sample_ternary_device.argtypes = [vp, vp, sz, vp, vp, vp]
    L.se_amd_sample_cbd_device.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    L.se_amd_word_ops_device.argtypes = [vp, sz, i32, vp, vp, vp, vp, sz, vp]
    L.se_amd_pack_ternary_host.argtypes = [vp, sz, vp]
    L.se_amd_pack_ternary_host.restype = None
    L.se_amd_pack_seal_ciphertext_host.argtypes = [vp, vp, sz, sz, vp]
    L.se_amd_pack_seal_ciphertext_host.restype = None
    L.se_amd_format_poly_text.argtypes = [C.c_char_p, vp, sz, vp, sz]
    L.se_amd_format_poly_text.restype = sz
    L.se_amd_format_values_text.argtypes = [C.c_char_p, vp, sz, vp, sz]
    L.se_amd_format_values_text.restype = sz
    L.se_amd_write_ciphertext_text.argtypes = [C.c_char_p, i32, vp, sz, vp, vp, sz, sz]
    L.se_amd_save_secret_key_file.argtypes = [C.c_char_p, sz, vp]
    L.se_amd_save_public_key_files.argtypes = [C.c_char_p, sz, sz, vp, vp, vp]
    L.se_amd_set_profiling.argtypes = [vp, i32]
    L.se_amd_stage_ms.argtypes = [vp, vp, vp, i32]
    L.se_amd_set_reject_list_capacity.argtypes = [vp, u32]
    L.se_amd_set_speculation_capacity.argtypes = [vp, u32]
    L.se_amd_set_host_chunk.argtypes = [vp, sz]
    L.se_amd_host_tables.argtypes = [sz, sz, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_ifft_table_sha256.argtypes = [vp, C.c_char_p]
    L.se_amd_reserve.argtypes = [vp, sz]
    L.se_amd_set_debug_flags.argtypes = [vp, u32]
    L.se_amd_set_pipeline.argtypes = [vp, i32, i32]
    L.se_amd_set_asym_chunks.argtypes = [vp, sz]
    L.se_amd_set_secret_keyring.argtypes = [vp, sz, vp]
    L.se_amd_set_public_keyring.argtypes = [vp, sz, vp, vp]
    L.se_amd_encrypt_sym_keyed_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_encrypt_asym_keyed_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_decrypt_decode_keyed_device.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp, vp]
    L.se_amd_decrypt_full_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.se_amd_decrypt_full_keyed_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp]
    L.se_amd_crt_constants.argtypes = [sz, sz, vp, vp]
    L.se_amd_ct_lincomb_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.se_amd_set_lincomb_split.argtypes = [vp, u32]
    L.se_amd_ct_rescale_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
    L.se_amd_ct_mul_plain_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp]
    L.se_amd_decrypt_level_device.argtypes = [vp, vp, vp, sz, sz, C.c_double, vp, vp, vp, vp, vp]
    L.se_amd_decrypt_level_keyed_device.argtypes = [vp, vp, vp, sz, sz, C.c_double, vp, vp, vp, vp, vp, vp]
    L.se_amd_rescale_constants.argtypes = [sz, sz, vp, vp]
    L.se_amd_ct_mul_device.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    L.se_amd_decrypt3_level_device.argtypes = [vp, vp, vp, vp, sz, sz, C.c_double, vp, vp, vp, vp, vp]
    L.se_amd_decrypt3_level_keyed_device.argtypes = [vp, vp, vp, vp, sz, sz, C.c_double, vp, vp, vp, vp, vp, vp]
    L.se_amd_gen_relin_key.argtypes = [vp, vp, vp, vp, vp, vp]
    L.se_amd_set_relin_key.argtypes = [vp, vp, vp]
    L.se_amd_ct_relin_device.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp]
    L.se_amd_galois_element.argtypes = [sz, C.c_int64, vp]
    L.se_amd_galois_table.argtypes = [sz, u32, vp]
    L.se_amd_gen_galois_keys.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp]
    L.se_amd_set_galois_keys.argtypes = [vp, vp, sz, vp, vp]
    L.se_amd_ct_galois_device.argtypes = [vp, vp, vp, sz, sz, u32, vp, vp, vp]
    L.se_amd_gen_relin_key_sp.argtypes = [vp, vp, vp, vp, vp, vp]
    L.se_amd_set_relin_key_sp.argtypes = [vp, vp, vp]
    L.se_amd_gen_galois_keys_sp.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp]
    L.se_amd_set_galois_keys_sp.argtypes = [vp, vp, sz, vp, vp]
    L.se_amd_ct_relin_sp_device.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp]
    L.se_amd_ct_galois_sp_device.argtypes = [vp, vp, vp, sz, sz, u32, vp, vp, vp]
    L.se_amd_ct_drop_primes_device.argtypes = [vp, vp, vp, sz, sz, sz, vp, vp, vp]
    L.se_amd_ct_galois_many_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]
    L.se_amd_ct_galois_sum_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, i32, vp, vp, vp]
    L.se_amd_lintrans_create.argtypes = [vp, vp, sz, vp, vp, sz, C.POINTER(vp)]
    L.se_amd_lintrans_destroy.argtypes = [vp]
    L.se_amd_lintrans_destroy.restype = None
    L.se_amd_ct_lintrans_device.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp]
    L.se_amd_ct_galois_sum_sp_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, i32, vp, vp, vp]
    L.se_amd_lintrans_create_sp.argtypes = [vp, vp, sz, vp, vp, sz, C.POINTER(vp)]
    L.se_amd_ct_lintrans_sp_device.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp]
    L.se_amd_ct_mul_plain_sum_device.argtypes = [vp, vp, vp, sz, sz, sz, vp, sz, sz, vp, vp, vp]
    L.se_amd_ct_galois_accum_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]
    L.se_amd_bsgs_create.argtypes = [vp, vp, sz, vp, sz, vp, sz, C.POINTER(vp)]
    L.se_amd_bsgs_destroy.argtypes = [vp]
    L.se_amd_bsgs_destroy.restype = None
    L.se_amd_bsgs_workspace_bytes.argtypes = [vp, sz, sz]
    L.se_amd_bsgs_workspace_bytes.restype = sz
    L.se_amd_ct_bsgs_device.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp, sz, vp]
    L.se_amd_ct_galois_many_ext_sp_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]
    L.se_amd_ct_mul_plain_sum_ext_sp_device.argtypes = [vp, vp, vp, sz, sz, sz, vp, sz, vp, vp, vp]
    L.se_amd_ct_mod_down_sp_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
    L.se_amd_ct_galois_accum_sp_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]
    L.se_amd_bsgs_create_sp.argtypes = [vp, vp, sz, vp, sz, vp, sz, C.POINTER(vp)]
    L.se_amd_ct_bsgs_sp_device.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp, sz, vp]
    L.se_amd_gen_switch_keys_sp.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.se_amd_set_switch_keyring_sp.argtypes = [vp, sz, vp, vp]
    L.se_amd_ct_switch_keyed_sp_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]
    L.se_amd_ct_switch_sum_keyed_sp_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp]
    L.se_amd_ct_pack_sp_device.argtypes = [vp, vp, vp, sz, sz, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.se_amd_ct_mul_sum_device.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.se_amd_ct_dot_sp_device.argtypes = [vp, vp, vp, sz, vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.se_amd_ct_affine_rescale_device.argtypes = [vp, vp, vp, vp, vp, sz, C.c_int64, sz, sz, vp, vp, vp]
    L.se_amd_poly_create.argtypes = [sz, sz, sz, vp, sz, C.c_double, C.c_double, C.POINTER(vp)]
    L.se_amd_poly_destroy.argtypes = [vp]
    L.se_amd_poly_destroy.restype = None
    L.se_amd_poly_terms.argtypes = [vp, vp, vp, vp, vp, sz]
    L.se_amd_poly_terms.restype = sz
    L.se_amd_poly_result.argtypes = [vp, vp, vp]
    L.se_amd_poly_workspace_bytes.argtypes = [vp, sz]
    L.se_amd_poly_workspace_bytes.restype = sz
    L.se_amd_ct_poly_sp_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp, vp, vp]
    _lib = L
    return L


def _check(rc, what):
    if rc < 0:
        msg = lib().se_amd_last_error().decode(errors="replace")
        raise SealEmbeddedAmdError(f"{what} failed with code {rc}: {msg}")
    return rc


def _ptr(t):
    """Device/host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        assert t.is_contiguous()
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host_tables(n, nprimes):
    """Setup-time tables computed on the host (no GPU needed): dict of numpy arrays."""
    import numpy as np
    L = lib()
    q = np.zeros(nprimes, np.uint32); cr = np.zeros((nprimes, 2), np.uint32)
    scale = C.c_double(0)
    imap = np.zeros(n, np.uint16); w = np.zeros((n, 2), np.float64)
    rw = np.zeros((nprimes, n, 2), np.uint32); irw = np.zeros_like(rw)
    _check(L.se_amd_host_tables(n, nprimes, _ptr(q), _ptr(cr), C.c_void_p(C.addressof(scale)), _ptr(imap), _ptr(w),
                                _ptr(rw), _ptr(irw)), "se_amd_host_tables")
    return dict(q=q, const_ratio=cr, scale=scale.value, index_map=imap, ifft_w=w, ntt_rw=rw, intt_rw=irw)


def crt_constants(n, nprimes):
    """Recombination constants of decrypt_full (host only): (inv, inv_shoup) uint32 [np], entry 0 unused."""
    import numpy as np
    inv = np.zeros(nprimes, np.uint32); sh = np.zeros(nprimes, np.uint32)
    _check(lib().se_amd_crt_constants(n, nprimes, _ptr(inv), _ptr(sh)), "se_amd_crt_constants")
    return inv, sh


def rescale_constants(n, primes):
    """Constants of the rescale from level `primes` (host only): (inv, inv_shoup) uint32 [primes - 1],
    inv[j] = q_{primes-1}^-1 mod q_j."""
    import numpy as np
    m = max(int(primes) - 1, 1)
    inv = np.zeros(m, np.uint32); sh = np.zeros(m, np.uint32)
    _check(lib().se_amd_rescale_constants(n, primes, _ptr(inv), _ptr(sh)), "se_amd_rescale_constants")
    return inv, sh


def galois_element(n, step):
    """The Galois element of a slot rotation (host only): 3^(step mod n/2) mod 2n.  It rotates the slot vector left by
    `step` (np.roll(v, -step)); a negative step rotates right; step 0 gives 1."""
    elt = C.c_uint32(0)
    _check(lib().se_amd_galois_element(n, int(step), C.c_void_p(C.addressof(elt))), "se_amd_galois_element")
    return int(elt.value)


def galois_table(n, elt):
    """The permutation of the automorphism x -> x^elt on an NTT-form row (host only): uint16 [n] with
    sigma(x)[k] = x[src[k]]."""
    import numpy as np
    src = np.zeros(n, np.uint16)
    _check(lib().se_amd_galois_table(n, int(elt), _ptr(src)), "se_amd_galois_table")
    return src


class _Plan:
    """Handle of a plan of the library; DESTROY names the symbol that frees it."""
    DESTROY = None

    def __init__(self, L, h):
        self.L, self.h = L, h

    def close(self):
        if self.h:
            getattr(self.L, self.DESTROY)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BsgsPlan(_Plan):
    """Handle of se_amd_bsgs_create (Context.bsgs_plan)."""
    DESTROY = "se_amd_bsgs_destroy"


class LintransPlan(_Plan):
    """Handle of se_amd_lintrans_create (Context.lintrans_plan)."""
    DESTROY = "se_amd_lintrans_destroy"


class PolyPlan(_Plan):
    """Handle of se_amd_poly_create (poly_create): the schedule of a slot-wise polynomial, host data only."""
    DESTROY = "se_amd_poly_destroy"

    def terms(self):
        """poly_terms(self)."""
        return poly_terms(self)

    def result(self):
        """poly_result(self)."""
        return poly_result(self)

    def workspace_bytes(self, records):
        return int(self.L.se_amd_poly_workspace_bytes(self.h, records))


def poly_create(n, nprimes, primes, coeff, scale_in, scale_out):
    """The plan of p(x) = sum coeff[d] x^d on level-`primes` records of the parameter set (n, nprimes) at scale scale_in,
    result at scale_out (host only: no context, no device).  The degree is len(coeff) - 1."""
    import numpy as np
    L = lib()
    a = np.ascontiguousarray(coeff, dtype=np.float64)
    h = C.c_void_p(None)
    _check(L.se_amd_poly_create(n, nprimes, primes, _ptr(a), len(a) - 1, scale_in, scale_out, C.byref(h)),
           "se_amd_poly_create")
    return PolyPlan(L, h)


def poly_terms(plan):
    """The needed powers of a plan in increasing order: list of dict(power, level, scale, weight), weight a Python int
    (0 for a power that is no term of the combine)."""
    import numpy as np
    cap = 16
    d = np.zeros(cap, np.uint32); lv = np.zeros(cap, np.uint32); sc = np.zeros(cap, np.float64); w = np.zeros(cap, np.int64)
    k = int(plan.L.se_amd_poly_terms(plan.h, _ptr(d), _ptr(lv), _ptr(sc), _ptr(w), cap))
    return [dict(power=int(d[i]), level=int(lv[i]), scale=float(sc[i]), weight=int(w[i])) for i in range(k)]


def poly_result(plan):
    """(out_primes, c_after) of a plan: the level of the result and the constant of the combine."""
    out_primes = C.c_size_t(0)
    c_after = C.c_int64(0)
    _check(plan.L.se_amd_poly_result(plan.h, C.c_void_p(C.addressof(out_primes)), C.c_void_p(C.addressof(c_after))),
           "se_amd_poly_result")
    return int(out_primes.value), int(c_after.value)


class Group:
    """One context per device of a node (se_amd_group): device-resident multi-GPU calls through the C ABI.
    `blocks` arguments are lists with one torch tensor per member, each on that member's device."""

    def __init__(self, n, nprimes, devices=None):
        self.L = lib()
        L = self.L
        L.se_amd_group_size.restype = C.c_size_t
        L.se_amd_group_ctx.restype = C.c_void_p
        L.se_amd_group_ctx.argtypes = [C.c_void_p, C.c_size_t]
        L.se_amd_group_destroy.restype = None
        L.se_amd_group_destroy.argtypes = [C.c_void_p]
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices) if devices else None
        _check(L.se_amd_group_create(C.byref(h), C.c_size_t(n), C.c_size_t(nprimes), arr,
                                     C.c_size_t(len(devices) if devices else 0)), "se_amd_group_create")
        self.h, self.n, self.np = h, n, nprimes
        self.size = int(L.se_amd_group_size(h))
        self.devices = [int(L.se_amd_group_device(h, C.c_size_t(i))) for i in range(self.size)]

    def close(self):
        if getattr(self, "h", None):
            self.L.se_amd_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def partition(self, B):
        first = (C.c_size_t * self.size)()
        count = (C.c_size_t * self.size)()
        _check(self.L.se_amd_group_partition(self.h, C.c_size_t(B), first, count), "se_amd_group_partition")
        return list(first), list(count)

    def set_secret_key(self, sk_packed):
        import numpy as np
        sk = np.ascontiguousarray(sk_packed, dtype=np.uint8)
        _check(self.L.se_amd_group_set_secret_key(self.h, _ptr(sk)), "se_amd_group_set_secret_key")

    def set_public_key(self, pk0, pk1):
        import numpy as np
        pk0 = np.ascontiguousarray(pk0, dtype=np.uint32)
        pk1 = np.ascontiguousarray(pk1, dtype=np.uint32)
        _check(self.L.se_amd_group_set_public_key(self.h, _ptr(pk0), _ptr(pk1)), "se_amd_group_set_public_key")

    def reserve(self, B):
        _check(self.L.se_amd_group_reserve(self.h, C.c_size_t(B)), "se_amd_group_reserve")

    def _arr(self, blocks):
        if blocks is None:
            return None
        assert len(blocks) == self.size
        return (C.c_void_p * self.size)(*[None if t is None else t.data_ptr() for t in blocks])

    def encrypt_sym(self, B, values, share_seeds, seeds, c0, c1=None, status=None, gather_root=-1, c0_all=None,
                    c1_all=None):
        _check(self.L.se_amd_encrypt_sym_multi_device(
            self.h, C.c_size_t(B), self._arr(values), self._arr(share_seeds), self._arr(seeds), self._arr(c0),
            self._arr(c1), self._arr(status), C.c_int(gather_root), _ptr(c0_all), _ptr(c1_all)),
            "se_amd_encrypt_sym_multi_device")

    def encrypt_asym(self, B, values, seeds, c0, c1, status=None, gather_root=-1, c0_all=None, c1_all=None):
        _check(self.L.se_amd_encrypt_asym_multi_device(
            self.h, C.c_size_t(B), self._arr(values), self._arr(seeds), self._arr(c0), self._arr(c1),
            self._arr(status), C.c_int(gather_root), _ptr(c0_all), _ptr(c1_all)),
            "se_amd_encrypt_asym_multi_device")

    def encode_ntt(self, B, values, out, status=None, gather_root=-1, out_all=None):
        _check(self.L.se_amd_encode_ntt_multi_device(
            self.h, C.c_size_t(B), self._arr(values), self._arr(out), self._arr(status), C.c_int(gather_root),
            _ptr(out_all)), "se_amd_encode_ntt_multi_device")


class Context:
    """One parameter set on one GPU (se_amd_ctx).  All tensors are torch CUDA tensors."""

    def __init__(self, n, nprimes, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.se_amd_create(C.byref(h), n, nprimes, device), "se_amd_create")
        self.h = h
        self.n, self.np, self.device = n, nprimes, device

    def close(self):
        if getattr(self, "h", None):
            self.L.se_amd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters / keys
    def scale(self):
        return float(self.L.se_amd_scale(self.h))

    def moduli(self):
        import numpy as np
        q = np.zeros(self.np, dtype=np.uint32)
        _check(self.L.se_amd_moduli(self.h, _ptr(q)), "se_amd_moduli")
        return [int(x) for x in q]

    def index_map(self):
        import numpy as np
        m = np.zeros(self.n, dtype=np.uint16)
        _check(self.L.se_amd_index_map(self.h, _ptr(m)), "se_amd_index_map")
        return m

    def ifft_table_sha256(self):
        """SHA-256 of the IFFT root table as the DEVICE holds it (SURVEY trap T8)."""
        buf = C.create_string_buffer(65)
        _check(self.L.se_amd_ifft_table_sha256(self.h, buf), "se_amd_ifft_table_sha256")
        return buf.value.decode()

    def set_secret_key(self, sk_packed):
        import numpy as np
        sk = np.ascontiguousarray(sk_packed, dtype=np.uint8)
        assert sk.size == self.n // 4
        _check(self.L.se_amd_set_secret_key(self.h, _ptr(sk)), "se_amd_set_secret_key")

    def set_public_key(self, pk0, pk1):
        import numpy as np
        pk0 = np.ascontiguousarray(pk0, dtype=np.uint32)
        pk1 = np.ascontiguousarray(pk1, dtype=np.uint32)
        assert pk0.size == self.np * self.n == pk1.size
        _check(self.L.se_amd_set_public_key(self.h, _ptr(pk0), _ptr(pk1)), "se_amd_set_public_key")

    def gen_public_key(self, sk_packed, pk_seed, ep_seed):
        import numpy as np
        sk = np.ascontiguousarray(sk_packed, dtype=np.uint8)
        s1 = np.frombuffer(bytes(pk_seed), dtype=np.uint8).copy()
        s2 = np.frombuffer(bytes(ep_seed), dtype=np.uint8).copy()
        pk0 = np.zeros((self.np, self.n), dtype=np.uint32)
        pk1 = np.zeros_like(pk0)
        _check(self.L.se_amd_gen_public_key(self.h, _ptr(sk), _ptr(s1), _ptr(s2), _ptr(pk0),
                                            _ptr(pk1)), "se_amd_gen_public_key")
        return pk0, pk1

    def gen_keys_batch(self, pk_seeds, ep_seeds, sk_seeds=None, sk_in=None):
        """K key pairs in one launch chain: (sk [K][n/4] uint8, pk0, pk1 [K][np][n] uint32)."""
        import numpy as np
        pks = np.ascontiguousarray(pk_seeds, dtype=np.uint8).reshape(-1, 64)
        K = pks.shape[0]
        eps = np.ascontiguousarray(ep_seeds, dtype=np.uint8).reshape(K, 64)
        sks = None if sk_seeds is None else np.ascontiguousarray(sk_seeds, dtype=np.uint8).reshape(K, 64)
        ski = None if sk_in is None else np.ascontiguousarray(sk_in, dtype=np.uint8).reshape(K, self.n // 4)
        sk = np.zeros((K, self.n // 4), dtype=np.uint8)
        pk0 = np.zeros((K, self.np, self.n), dtype=np.uint32)
        pk1 = np.zeros_like(pk0)
        _check(self.L.se_amd_gen_keys_batch(self.h, K, _ptr(ski), _ptr(sks), _ptr(pks), _ptr(eps), _ptr(sk),
                                            _ptr(pk0), _ptr(pk1)), "se_amd_gen_keys_batch")
        return sk, pk0, pk1

    # ---- key rings (K keys; the keyed entries choose one per ciphertext)
    def set_secret_keyring(self, sk_packed):
        """sk_packed [K][n/4] uint8 (as gen_keys_batch returns it)."""
        import numpy as np
        sk = np.ascontiguousarray(sk_packed, dtype=np.uint8).reshape(-1, self.n // 4)
        _check(self.L.se_amd_set_secret_keyring(self.h, sk.shape[0], _ptr(sk)), "se_amd_set_secret_keyring")

    def set_public_keyring(self, pk0, pk1):
        """pk0, pk1 [K][np][n] uint32 in NTT form (as gen_keys_batch returns them)."""
        import numpy as np
        pk0 = np.ascontiguousarray(pk0, dtype=np.uint32).reshape(-1, self.np, self.n)
        pk1 = np.ascontiguousarray(pk1, dtype=np.uint32).reshape(-1, self.np, self.n)
        assert pk0.shape == pk1.shape
        _check(self.L.se_amd_set_public_keyring(self.h, pk0.shape[0], _ptr(pk0), _ptr(pk1)),
               "se_amd_set_public_keyring")

    def load_keys_from_dir(self, path, want_pk=False):
        _check(self.L.se_amd_load_keys_from_dir(self.h, path.encode(), 1 if want_pk else 0),
               "se_amd_load_keys_from_dir")

    # ---- whole path (device tensors, async on torch's current stream)
    def encrypt_sym(self, values, share_seeds, seeds, c0, c1, ntt_pte=None, pte=None, status=None):
        B = values.shape[0]
        _check(self.L.se_amd_encrypt_sym_device(self.h, _ptr(values), B, _ptr(share_seeds),
                                                _ptr(seeds), _ptr(c0), _ptr(c1), _ptr(ntt_pte),
                                                _ptr(pte), _ptr(status), _stream_ptr()),
               "se_amd_encrypt_sym_device")

    def encrypt_sym_seeded(self, values, share_seeds, seeds, c0, status=None):
        _check(self.L.se_amd_encrypt_sym_seeded_device(self.h, _ptr(values), values.shape[0],
                                                       _ptr(share_seeds), _ptr(seeds), _ptr(c0),
                                                       _ptr(status), _stream_ptr()),
               "se_amd_encrypt_sym_seeded_device")

    def expand_c1(self, share_seeds, c1):
        _check(self.L.se_amd_expand_c1_device(self.h, _ptr(share_seeds), share_seeds.shape[0],
                                              _ptr(c1), _stream_ptr()), "se_amd_expand_c1_device")

    def encrypt_asym(self, values, seeds, c0, c1, ntt_pte=None, pte=None, status=None):
        B = values.shape[0]
        _check(self.L.se_amd_encrypt_asym_device(self.h, _ptr(values), B, _ptr(seeds), _ptr(c0),
                                                 _ptr(c1), _ptr(ntt_pte), _ptr(pte), _ptr(status),
                                                 _stream_ptr()), "se_amd_encrypt_asym_device")

    def encrypt_sym_keyed(self, values, key_idx, share_seeds, seeds, c0, c1=None, ntt_pte=None, pte=None,
                          status=None):
        """Ciphertext b under secret-ring key key_idx[b] (int32/uint32 device tensor [B]); c1=None gives the
        seed-compressed form.  Status 2: key_idx[b] >= K (c0 zero)."""
        B = values.shape[0]
        _check(self.L.se_amd_encrypt_sym_keyed_device(self.h, _ptr(values), B, _ptr(key_idx), _ptr(share_seeds),
                                                      _ptr(seeds), _ptr(c0), _ptr(c1), _ptr(ntt_pte), _ptr(pte),
                                                      _ptr(status), _stream_ptr()),
               "se_amd_encrypt_sym_keyed_device")

    def encrypt_asym_keyed(self, values, key_idx, seeds, c0, c1, ntt_pte=None, pte=None, status=None):
        """Ciphertext b under public-ring key key_idx[b]; status 2: key_idx[b] >= K (c0, c1 zero)."""
        B = values.shape[0]
        _check(self.L.se_amd_encrypt_asym_keyed_device(self.h, _ptr(values), B, _ptr(key_idx), _ptr(seeds),
                                                       _ptr(c0), _ptr(c1), _ptr(ntt_pte), _ptr(pte), _ptr(status),
                                                       _stream_ptr()), "se_amd_encrypt_asym_keyed_device")

    def encode_ntt(self, values, out, pte=None, status=None):
        B = values.shape[0]
        _check(self.L.se_amd_encode_ntt_device(self.h, _ptr(values), B, _ptr(out), _ptr(pte),
                                               _ptr(status), _stream_ptr()),
               "se_amd_encode_ntt_device")

    # ---- stage level
    def encode(self, values, out, status=None):
        _check(self.L.se_amd_encode_device(self.h, _ptr(values), values.shape[0], _ptr(out),
                                           _ptr(status), _stream_ptr()), "se_amd_encode_device")

    def ntt(self, prime, polys):
        count = polys.numel() // self.n
        _check(self.L.se_amd_ntt_device(self.h, prime, _ptr(polys), count, _stream_ptr()),
               "se_amd_ntt_device")

    def intt(self, prime, polys):
        count = polys.numel() // self.n
        _check(self.L.se_amd_intt_device(self.h, prime, _ptr(polys), count, _stream_ptr()),
               "se_amd_intt_device")

    def decrypt_decode(self, c0, c1, prime, dec_ntt=None, pt=None, values=None):
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt_decode_device(self.h, _ptr(c0), _ptr(c1), B, prime,
                                                   _ptr(dec_ntt), _ptr(pt), _ptr(values),
                                                   _stream_ptr()), "se_amd_decrypt_decode_device")

    def decrypt_decode_keyed(self, c0, c1, key_idx, prime, dec_ntt=None, pt=None, values=None):
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt_decode_keyed_device(self.h, _ptr(c0), _ptr(c1), B, _ptr(key_idx), prime,
                                                         _ptr(dec_ntt), _ptr(pt), _ptr(values), _stream_ptr()),
               "se_amd_decrypt_decode_keyed_device")

    def decrypt_full(self, c0, c1, pte=None, values=None, values_f64=None, status=None):
        """All primes recombined: pte int64 [B][n], values float32 / values_f64 float64 [B][n/2], status uint8 [B]
        (1 = every coefficient fits int64); each optional, at least one required."""
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt_full_device(self.h, _ptr(c0), _ptr(c1), B, _ptr(pte), _ptr(values),
                                                 _ptr(values_f64), _ptr(status), _stream_ptr()),
               "se_amd_decrypt_full_device")

    def decrypt_full_keyed(self, c0, c1, key_idx, pte=None, values=None, values_f64=None, status=None):
        """decrypt_full with ciphertext b under secret-ring key key_idx[b]; status 2 and zero outputs for an
        index >= K."""
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt_full_keyed_device(self.h, _ptr(c0), _ptr(c1), B, _ptr(key_idx), _ptr(pte),
                                                       _ptr(values), _ptr(values_f64), _ptr(status), _stream_ptr()),
               "se_amd_decrypt_full_keyed_device")

    def ct_lincomb(self, in0, out0, in1=None, out1=None, row_ptr=None, idx=None, w=None, G=None, status=None):
        """Key-free weighted sums of records: out[g] = sum_k (w_k mod q) . in[idx_k] mod q on one or two slabs
        [B][np][n].  CSR form: row_ptr [G+1], idx [nnz] (uint32 / int32 bits), w [nnz] int32 or None for all ones.
        Dense form (row_ptr = idx = None): w [G][B], or None with G = 1 for the plain sum.  status uint8 [G]:
        2 and a zero row for an index >= B or a bad row_ptr pair."""
        B = in0.shape[0]
        if row_ptr is not None:
            G = row_ptr.numel() - 1
            nnz = idx.numel() if idx is not None else 0
        else:
            if G is None:
                G = w.shape[0] if w is not None else 1
            nnz = G * B
        _check(self.L.se_amd_ct_lincomb_device(self.h, _ptr(in0), _ptr(in1), B, G, _ptr(row_ptr), _ptr(idx), _ptr(w),
                                               nnz, _ptr(out0), _ptr(out1), _ptr(status), _stream_ptr()),
               "se_amd_ct_lincomb_device")

    def set_lincomb_split(self, S):
        """Test hook: slices a row of ct_lincomb is cut into (0 = automatic); every value gives the same bits."""
        _check(self.L.se_amd_set_lincomb_split(self.h, S), "se_amd_set_lincomb_split")

    def ct_rescale(self, in0, out0, in1=None, out1=None, primes=None):
        """Key-free rescale of one or two slabs [B][primes][n] -> [B][primes-1][n] (out rows of B records, packed):
        the exact quotient (c - delta) / q_last, delta = c mod q_last centred.  primes defaults to in0.shape[1]."""
        B = in0.shape[0]
        if primes is None:
            primes = in0.shape[1]
        _check(self.L.se_amd_ct_rescale_device(self.h, _ptr(in0), _ptr(in1), B, primes, _ptr(out0), _ptr(out1),
                                               _stream_ptr()), "se_amd_ct_rescale_device")

    def ct_mul_plain(self, in0, pt, out0, in1=None, out1=None, pt_idx=None, primes=None, status=None):
        """Key-free slot-wise product of one or two slabs [B][primes][n] with encoded plaintexts pt [P][pt_primes][n]
        (encode_ntt's layout): record b times plaintext pt_idx[b], or with pt_idx=None the one plaintext (P = 1) or
        plaintext b (P = B).  status uint8 [B]: 2 and zero rows for an index >= P.  out may be the input itself."""
        B = in0.shape[0]
        if primes is None:
            primes = in0.shape[1]
        _check(self.L.se_amd_ct_mul_plain_device(self.h, _ptr(in0), _ptr(in1), B, primes, _ptr(pt), pt.shape[0],
                                                 pt.shape[1], _ptr(pt_idx), _ptr(out0), _ptr(out1), _ptr(status),
                                                 _stream_ptr()), "se_amd_ct_mul_plain_device")

    def decrypt_level(self, c0, c1, primes, scale, pte=None, values=None, values_f64=None, status=None):
        """decrypt_full on records of `primes` <= np primes [B][primes][n], decoded with `scale`."""
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt_level_device(self.h, _ptr(c0), _ptr(c1), B, primes, scale, _ptr(pte),
                                                  _ptr(values), _ptr(values_f64), _ptr(status), _stream_ptr()),
               "se_amd_decrypt_level_device")

    def decrypt_level_keyed(self, c0, c1, key_idx, primes, scale, pte=None, values=None, values_f64=None,
                            status=None):
        """decrypt_level with ciphertext b under secret-ring key key_idx[b]; status 2 and zero outputs for an
        index >= K."""
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt_level_keyed_device(self.h, _ptr(c0), _ptr(c1), B, primes, scale, _ptr(key_idx),
                                                        _ptr(pte), _ptr(values), _ptr(values_f64), _ptr(status),
                                                        _stream_ptr()), "se_amd_decrypt_level_keyed_device")

    def ct_mul(self, a0, a1, b0, b1, out0, out1, out2, ia=None, ib=None, primes=None, status=None):
        """Key-free tensor product: pair p = record ia[p] of (a0, a1) times record ib[p] of (b0, b1), slabs
        [B][primes][n]; out0 = x0 y0, out1 = x0 y1 + x1 y0, out2 = x1 y1, each [P][primes][n].  ia = ib = None: pair p is
        (p, p) and both sides hold P records.  status uint8 [P]: 2 and zero rows for an index out of range."""
        if primes is None:
            primes = a0.shape[1]
        P = ia.numel() if ia is not None else a0.shape[0]
        _check(self.L.se_amd_ct_mul_device(self.h, _ptr(a0), _ptr(a1), a0.shape[0], _ptr(b0), _ptr(b1), b0.shape[0],
                                           primes, P, _ptr(ia), _ptr(ib), _ptr(out0), _ptr(out1), _ptr(out2),
                                           _ptr(status), _stream_ptr()), "se_amd_ct_mul_device")

    def _mul_sum_shape(self, a0, row_ptr, ia, primes):
        """(primes, G, nnz) of a grouped product call: ia = ib = None is the identity pair list over the whole batch."""
        return (a0.shape[1] if primes is None else primes, row_ptr.numel() - 1,
                ia.numel() if ia is not None else a0.shape[0])

    def ct_mul_sum(self, a0, a1, b0, b1, row_ptr, ia, ib, out0, out1, out2, primes=None, status=None):
        """Key-free grouped product sums: output row g = the sum over k in [row_ptr[g], row_ptr[g + 1]) of the tensor of
        record ia[k] of (a0, a1) and record ib[k] of (b0, b1) (ia = ib = None: pair k is (k, k)); out0, out1, out2 are
        [G][primes][n].  The bits of ct_mul on the pairs and unweighted ct_lincomb row sums, without the per-pair
        record.  status uint8 [G]: 2 and a zero row for a pair index out of range or a bad row_ptr pair."""
        primes, G, nnz = self._mul_sum_shape(a0, row_ptr, ia, primes)
        _check(self.L.se_amd_ct_mul_sum_device(self.h, _ptr(a0), _ptr(a1), a0.shape[0], _ptr(b0), _ptr(b1), b0.shape[0],
                                               primes, G, _ptr(row_ptr), _ptr(ia), _ptr(ib), nnz, _ptr(out0),
                                               _ptr(out1), _ptr(out2), _ptr(status), _stream_ptr()),
               "se_amd_ct_mul_sum_device")

    def ct_dot_sp(self, a0, a1, b0, b1, row_ptr, ia, ib, out0, out1, primes=None, status=None):
        """Encrypted inner products: the rows of ct_mul_sum relinearised under the installed special-prime key inside the
        same launch, ONE key switch and one division by the special prime per row; primes <= np - 1, out0, out1 are
        [G][primes][n] at the product's scale and the operands' level.  The bits of ct_mul_sum followed by ct_relin_sp,
        with the tensor sums never in memory.  status as ct_mul_sum."""
        primes, G, nnz = self._mul_sum_shape(a0, row_ptr, ia, primes)
        _check(self.L.se_amd_ct_dot_sp_device(self.h, _ptr(a0), _ptr(a1), a0.shape[0], _ptr(b0), _ptr(b1), b0.shape[0],
                                              primes, G, _ptr(row_ptr), _ptr(ia), _ptr(ib), nnz, _ptr(out0), _ptr(out1),
                                              _ptr(status), _stream_ptr()), "se_amd_ct_dot_sp_device")

    def ct_affine_rescale(self, terms0, terms1, w, c_after, out0, out1, primes):
        """Key-free weighted sum of T <= 16 term records at their own levels, ONE rescale and a constant: terms0 / terms1
        are lists of device slabs [B][term_primes][n] (term_primes = shape[1] >= primes, the first `primes` rows are read),
        w a list of Python ints within int64, c_after an int within int64 added to slab 0 after the rescale; out0, out1
        are [B][primes - 1][n].  The bits of ct_drop_primes per term, the weighted modular sum, ct_rescale and the
        constant, without the copies and the sum in memory."""
        import numpy as np
        T = len(terms0)
        p0 = (C.c_void_p * T)(*[t.data_ptr() for t in terms0])
        p1 = (C.c_void_p * T)(*[t.data_ptr() for t in terms1])
        assert all(t.is_contiguous() for t in list(terms0) + list(terms1))
        tp = np.array([t.shape[1] for t in terms0], dtype=np.uint32)
        wv = np.array([int(x) for x in w], dtype=np.int64)
        _check(self.L.se_amd_ct_affine_rescale_device(self.h, p0, p1, _ptr(tp), _ptr(wv), T, int(c_after),
                                                      terms0[0].shape[0], primes, _ptr(out0), _ptr(out1), _stream_ptr()),
               "se_amd_ct_affine_rescale_device")

    def poly_workspace_bytes(self, plan, records):
        """Bytes of device workspace a ct_poly_sp call of `plan` on `records` records needs."""
        return plan.workspace_bytes(records)

    def ct_poly_sp(self, plan, c0, c1, out0, out1, workspace, workspace_bytes=None):
        """p(x) slot-wise on level-L records [B][L][n] under the installed special-prime relinearisation key, by the
        schedule of `plan` (poly_create) in the caller's `workspace` (a device tensor of at least plan.workspace_bytes(B)
        bytes; None for a plan of degree 1): the ladder of one-pair ct_dot_sp rows and rescales, then one
        ct_affine_rescale.  out0, out1 are [B][plan.result()[0]][n] at scale_out."""
        if workspace_bytes is None:
            workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
        _check(self.L.se_amd_ct_poly_sp_device(self.h, plan.h, _ptr(c0), _ptr(c1), c0.shape[0], _ptr(workspace),
                                               workspace_bytes, _ptr(out0), _ptr(out1), _stream_ptr()),
               "se_amd_ct_poly_sp_device")

    def decrypt3_level(self, c0, c1, c2, primes, scale, pte=None, values=None, values_f64=None, status=None):
        """decrypt_level on the degree-2 form (c0, c1, c2): d = c0 + s (c1 + s c2) per prime."""
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt3_level_device(self.h, _ptr(c0), _ptr(c1), _ptr(c2), B, primes, scale, _ptr(pte),
                                                   _ptr(values), _ptr(values_f64), _ptr(status), _stream_ptr()),
               "se_amd_decrypt3_level_device")

    def decrypt3_level_keyed(self, c0, c1, c2, key_idx, primes, scale, pte=None, values=None, values_f64=None,
                             status=None):
        """decrypt3_level with record b under secret-ring key key_idx[b]; status 2 and zero outputs for an
        index >= K."""
        B = c0.shape[0]
        _check(self.L.se_amd_decrypt3_level_keyed_device(self.h, _ptr(c0), _ptr(c1), _ptr(c2), B, primes, scale,
                                                         _ptr(key_idx), _ptr(pte), _ptr(values), _ptr(values_f64),
                                                         _ptr(status), _stream_ptr()),
               "se_amd_decrypt3_level_keyed_device")

    def _evk_gen_buffers(self, sk_packed, a_seeds, e_seeds, lead=(), R=None):
        """What generating evaluation keys takes and fills: the packed key, the seed blocks lead + [R][64] and two
        zeroed key halves lead + [R][np][n], R = 2 np (a special-prime key: R = np - 1)."""
        import numpy as np
        R = 2 * self.np if R is None else R
        sk = np.ascontiguousarray(sk_packed, dtype=np.uint8)
        assert sk.size == self.n // 4
        sa = np.ascontiguousarray(a_seeds, dtype=np.uint8).reshape(*lead, R, 64)
        se = np.ascontiguousarray(e_seeds, dtype=np.uint8).reshape(*lead, R, 64)
        k0 = np.zeros((*lead, R, self.np, self.n), dtype=np.uint32)
        return sk, sa, se, k0, np.zeros_like(k0)

    def _evk_halves(self, k0, k1, count=1, R=None):
        """The two halves of `count` evaluation keys as contiguous uint32, [count][R][np][n] words each, R = 2 np (a
        special-prime key: R = np - 1)."""
        import numpy as np
        R = 2 * self.np if R is None else R
        k0 = np.ascontiguousarray(k0, dtype=np.uint32)
        k1 = np.ascontiguousarray(k1, dtype=np.uint32)
        assert k0.size == count * R * self.np * self.n == k1.size
        return k0, k1

    def gen_relin_key(self, sk_packed, a_seeds, e_seeds):
        """Relinearisation key of sk_packed from R = 2 np seed pairs [R][64]: (evk0, evk1) uint32 [R][np][n]."""
        sk, sa, se, evk0, evk1 = self._evk_gen_buffers(sk_packed, a_seeds, e_seeds)
        _check(self.L.se_amd_gen_relin_key(self.h, _ptr(sk), _ptr(sa), _ptr(se), _ptr(evk0), _ptr(evk1)),
               "se_amd_gen_relin_key")
        return evk0, evk1

    def set_relin_key(self, evk0, evk1):
        """evk0, evk1 [2 np][np][n] uint32 (as gen_relin_key returns them); a word >= q_i is refused."""
        evk0, evk1 = self._evk_halves(evk0, evk1)
        _check(self.L.se_amd_set_relin_key(self.h, _ptr(evk0), _ptr(evk1)), "se_amd_set_relin_key")

    def ct_relin(self, d0, d1, d2, out0, out1, primes=None):
        """Relinearisation of the degree-2 form (d0, d1, d2) [B][primes][n] with the installed key -> (out0, out1) of
        the same level; no secret key is needed."""
        if primes is None:
            primes = d0.shape[1]
        _check(self.L.se_amd_ct_relin_device(self.h, _ptr(d0), _ptr(d1), _ptr(d2), d0.shape[0], primes, _ptr(out0),
                                             _ptr(out1), _stream_ptr()), "se_amd_ct_relin_device")

    def gen_galois_keys(self, sk_packed, elts, a_seeds, e_seeds):
        """Galois keys of sk_packed for the elements `elts` (odd, below 2n) from G blocks of R = 2 np seed pairs
        [G][R][64]: (gk0, gk1) uint32 [G][R][np][n]."""
        import numpy as np
        el = np.ascontiguousarray(elts, dtype=np.uint32).reshape(-1)
        G = el.size
        sk, sa, se, gk0, gk1 = self._evk_gen_buffers(sk_packed, a_seeds, e_seeds, lead=(G,))
        _check(self.L.se_amd_gen_galois_keys(self.h, _ptr(sk), _ptr(el), G, _ptr(sa), _ptr(se), _ptr(gk0), _ptr(gk1)),
               "se_amd_gen_galois_keys")
        return gk0, gk1

    def set_galois_keys(self, elts, gk0, gk1):
        """elts [G], gk0, gk1 [G][2 np][np][n] uint32 (as gen_galois_keys returns them): replaces the installed set; a
        word >= q_i, an even or repeated element is refused and the previous set stays."""
        import numpy as np
        el = np.ascontiguousarray(elts, dtype=np.uint32).reshape(-1)
        gk0, gk1 = self._evk_halves(gk0, gk1, el.size)
        _check(self.L.se_amd_set_galois_keys(self.h, _ptr(el), el.size, _ptr(gk0), _ptr(gk1)),
               "se_amd_set_galois_keys")

    def ct_galois(self, c0, c1, elt, out0, out1, primes=None):
        """The automorphism x -> x^elt on the records (c0, c1) [B][primes][n] and its key switch with the installed
        Galois key of `elt` -> (out0, out1) of the same level under the same key; no secret key is needed.
        elt = galois_element(n, s) rotates the slots left by s."""
        if primes is None:
            primes = c0.shape[1]
        _check(self.L.se_amd_ct_galois_device(self.h, _ptr(c0), _ptr(c1), c0.shape[0], primes, int(elt), _ptr(out0),
                                              _ptr(out1), _stream_ptr()), "se_amd_ct_galois_device")

    # ---- special-prime (hybrid) key switch: the last prime of the context belongs to the key, records have at most
    # np - 1 primes; keys of R' = np - 1 rows, installed sets of their own beside the digit keys
    def gen_relin_key_sp(self, sk_packed, a_seeds, e_seeds):
        """Special-prime relinearisation key of sk_packed from R' = np - 1 seed pairs [R'][64]: (evk0, evk1) uint32
        [R'][np][n]."""
        sk, sa, se, evk0, evk1 = self._evk_gen_buffers(sk_packed, a_seeds, e_seeds, R=max(self.np - 1, 1))
        _check(self.L.se_amd_gen_relin_key_sp(self.h, _ptr(sk), _ptr(sa), _ptr(se), _ptr(evk0), _ptr(evk1)),
               "se_amd_gen_relin_key_sp")
        return evk0, evk1

    def set_relin_key_sp(self, evk0, evk1):
        """evk0, evk1 [np - 1][np][n] uint32 (as gen_relin_key_sp returns them); a word >= q_i is refused."""
        evk0, evk1 = self._evk_halves(evk0, evk1, R=max(self.np - 1, 1))
        _check(self.L.se_amd_set_relin_key_sp(self.h, _ptr(evk0), _ptr(evk1)), "se_amd_set_relin_key_sp")

    def ct_relin_sp(self, d0, d1, d2, out0, out1, primes=None):
        """Relinearisation of (d0, d1, d2) [B][primes][n], primes <= np - 1, with the installed special-prime key ->
        (out0, out1) of the same level and scale: the key-switch term is divided by the last prime of the context."""
        if primes is None:
            primes = d0.shape[1]
        _check(self.L.se_amd_ct_relin_sp_device(self.h, _ptr(d0), _ptr(d1), _ptr(d2), d0.shape[0], primes, _ptr(out0),
                                                _ptr(out1), _stream_ptr()), "se_amd_ct_relin_sp_device")

    def gen_galois_keys_sp(self, sk_packed, elts, a_seeds, e_seeds):
        """Special-prime Galois keys of sk_packed for `elts` from G blocks of R' = np - 1 seed pairs [G][R'][64]: (gk0,
        gk1) uint32 [G][R'][np][n]."""
        import numpy as np
        el = np.ascontiguousarray(elts, dtype=np.uint32).reshape(-1)
        G = el.size
        sk, sa, se, gk0, gk1 = self._evk_gen_buffers(sk_packed, a_seeds, e_seeds, lead=(G,), R=max(self.np - 1, 1))
        _check(self.L.se_amd_gen_galois_keys_sp(self.h, _ptr(sk), _ptr(el), G, _ptr(sa), _ptr(se), _ptr(gk0),
                                                _ptr(gk1)), "se_amd_gen_galois_keys_sp")
        return gk0, gk1

    def set_galois_keys_sp(self, elts, gk0, gk1):
        """elts [G], gk0, gk1 [G][np - 1][np][n] uint32: replaces the installed special-prime set (the digit set is not
        touched); refusals as set_galois_keys."""
        import numpy as np
        el = np.ascontiguousarray(elts, dtype=np.uint32).reshape(-1)
        gk0, gk1 = self._evk_halves(gk0, gk1, el.size, R=max(self.np - 1, 1))
        _check(self.L.se_amd_set_galois_keys_sp(self.h, _ptr(el), el.size, _ptr(gk0), _ptr(gk1)),
               "se_amd_set_galois_keys_sp")

    def ct_galois_sp(self, c0, c1, elt, out0, out1, primes=None):
        """ct_galois with the installed special-prime Galois key of `elt` on records (c0, c1) [B][primes][n], primes <=
        np - 1: a rotation at the record's own scale, no lift and no rescale."""
        if primes is None:
            primes = c0.shape[1]
        _check(self.L.se_amd_ct_galois_sp_device(self.h, _ptr(c0), _ptr(c1), c0.shape[0], primes, int(elt),
                                                 _ptr(out0), _ptr(out1), _stream_ptr()), "se_amd_ct_galois_sp_device")

    def ct_drop_primes(self, in0, out0, in1=None, out1=None, primes_in=None, primes_out=None):
        """Rows 0 .. primes_out-1 of every record of one or two slabs [B][primes_in][n] -> [B][primes_out][n] (a device
        copy); primes_in defaults to in0.shape[1], primes_out to primes_in - 1."""
        if primes_in is None:
            primes_in = in0.shape[1]
        if primes_out is None:
            primes_out = primes_in - 1
        _check(self.L.se_amd_ct_drop_primes_device(self.h, _ptr(in0), _ptr(in1), in0.shape[0], primes_in, primes_out,
                                                   _ptr(out0), _ptr(out1), _stream_ptr()),
               "se_amd_ct_drop_primes_device")

    # ---- switch-key rings: K special-prime keys that hide P . s_from_k under s_to; record b is switched under ring key
    # key_idx[b].  The generator needs both secrets (the authority that issued the keys); the ring is public material
    def gen_switch_keys_sp(self, sk_from, sk_to, a_seeds, e_seeds):
        """Switching keys from the K packed keys sk_from [K][n/4] to sk_to [n/4], from K blocks of R' = np - 1 seed pairs
        [K][R'][64]: (wk0, wk1) uint32 [K][R'][np][n].  Installs nothing."""
        import numpy as np
        R = max(self.np - 1, 1)
        skf = np.ascontiguousarray(sk_from, dtype=np.uint8).reshape(-1, self.n // 4)
        K = skf.shape[0]
        skt = np.ascontiguousarray(sk_to, dtype=np.uint8)
        assert skt.size == self.n // 4
        sa = np.ascontiguousarray(a_seeds, dtype=np.uint8).reshape(K, R, 64)
        se = np.ascontiguousarray(e_seeds, dtype=np.uint8).reshape(K, R, 64)
        wk0 = np.zeros((K, R, self.np, self.n), dtype=np.uint32)
        wk1 = np.zeros_like(wk0)
        _check(self.L.se_amd_gen_switch_keys_sp(self.h, K, _ptr(skf), _ptr(skt), _ptr(sa), _ptr(se), _ptr(wk0),
                                                _ptr(wk1)), "se_amd_gen_switch_keys_sp")
        return wk0, wk1

    def set_switch_keyring_sp(self, wk0, wk1):
        """wk0, wk1 [K][np - 1][np][n] uint32 (as gen_switch_keys_sp returns them): replaces the installed switch ring; a
        word >= q_i is refused and the previous ring stays."""
        import numpy as np
        R = max(self.np - 1, 1)
        wk0 = np.ascontiguousarray(wk0, dtype=np.uint32)
        K = wk0.size // (R * self.np * self.n)
        wk0, wk1 = self._evk_halves(wk0, wk1, K, R=R)
        _check(self.L.se_amd_set_switch_keyring_sp(self.h, K, _ptr(wk0), _ptr(wk1)), "se_amd_set_switch_keyring_sp")

    def ct_switch_keyed_sp(self, c0, c1, key_idx, out0, out1, primes=None, status=None):
        """Record b of (c0, c1) [B][primes][n], primes <= np - 1, from the key of ring entry key_idx[b] to the ring's
        target key, at the record's own scale: the bits of ct_relin_sp(c0, 0, c1) under that ring key.  status uint8 [B]:
        2 and zero rows for an index >= K."""
        if primes is None:
            primes = c0.shape[1]
        _check(self.L.se_amd_ct_switch_keyed_sp_device(self.h, _ptr(c0), _ptr(c1), c0.shape[0], primes, _ptr(key_idx),
                                                       _ptr(out0), _ptr(out1), _ptr(status), _stream_ptr()),
               "se_amd_ct_switch_keyed_sp_device")

    def ct_switch_sum_keyed_sp(self, c0, c1, key_idx, row_ptr, idx, out0, out1, primes=None, status=None):
        """Switch and sum: output row g = the sum of the records idx[row_ptr[g] .. row_ptr[g + 1]) of (c0, c1)
        [B][primes][n], each switched under ring key key_idx[b], with ONE division by the special prime per row; out0,
        out1 are [G][primes][n].  A row of one record has the bits of ct_switch_keyed_sp.  status uint8 [G]: 2 and a
        zero row for a record index >= B, a member's key index >= K or a bad row_ptr pair."""
        if primes is None:
            primes = c0.shape[1]
        G = row_ptr.numel() - 1
        nnz = idx.numel() if idx is not None else 0
        _check(self.L.se_amd_ct_switch_sum_keyed_sp_device(self.h, _ptr(c0), _ptr(c1), c0.shape[0], primes,
                                                           _ptr(key_idx), G, _ptr(row_ptr), _ptr(idx), nnz, _ptr(out0),
                                                           _ptr(out1), _ptr(status), _stream_ptr()),
               "se_amd_ct_switch_sum_keyed_sp_device")

    def ct_pack_sp(self, c0, c1, elts, eidx, out0, out1, primes=None, row_ptr=None, idx=None, status=None):
        """Slot packing: entry k = record idx[k] of (c0, c1) [B][primes][n], primes <= np - 1, rotated by the element
        elts[eidx[k]] (a host list; element 1 is the identity and needs no key) under the installed special-prime Galois
        keys; output row g = the sum of the entries row_ptr[g] .. row_ptr[g + 1] with ONE division by the special prime
        per row; out0, out1 are [G][primes][n].  row_ptr = idx = None: the single form, row g = record g under
        elts[eidx[g]], the bits of ct_galois_sp per record.  status uint8 [G]: 2 and a zero row for a record index >= B,
        an element index >= len(elts) or a bad row_ptr pair."""
        import numpy as np
        el = np.ascontiguousarray(elts, dtype=np.uint32).reshape(-1)
        if primes is None:
            primes = c0.shape[1]
        G = row_ptr.numel() - 1 if row_ptr is not None else c0.shape[0]
        _check(self.L.se_amd_ct_pack_sp_device(self.h, _ptr(c0), _ptr(c1), c0.shape[0], primes, _ptr(el), el.size, G,
                                               _ptr(row_ptr), _ptr(idx), _ptr(eidx), eidx.numel(), _ptr(out0),
                                               _ptr(out1), _ptr(status), _stream_ptr()),
               "se_amd_ct_pack_sp_device")

    # ---- the rotation family: one private helper per shape of call; the public methods name the symbol and what differs
    def _galois_set(self, sym, in0, in1, elts, out0, out1, primes, stacked=False, flags=()):
        """A call on a set of Galois elements: records [B][primes][n], or a stack [G][B][primes][n]; `flags` stand
        between the elements and the outputs."""
        import numpy as np
        el = np.ascontiguousarray(elts, dtype=np.uint32).reshape(-1)
        if primes is None:
            primes = in0.shape[2 if stacked else 1]
        _check(getattr(self.L, sym)(self.h, _ptr(in0), _ptr(in1), in0.shape[1 if stacked else 0], primes, _ptr(el),
                                    el.size, *flags, _ptr(out0), _ptr(out1), _stream_ptr()), sym)

    def _make_plan(self, cls, sym, lists, tensors, pt_primes):
        """A plan from host element lists and device diagonals."""
        import numpy as np
        els = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in lists]   # alive until the call returns
        args = [a for el in els for a in (_ptr(el), el.size)]
        h = C.c_void_p()
        _check(getattr(self.L, sym)(self.h, *args, *[_ptr(t) for t in tensors], pt_primes, C.byref(h)), sym)
        return cls(self.L, h)

    def _plan_call(self, sym, plan, c0, c1, out0, out1, primes, tail=()):
        """A plan's call on the records (c0, c1) [B][primes][n]; `tail` stands between the outputs and the stream."""
        if primes is None:
            primes = c0.shape[1]
        _check(getattr(self.L, sym)(self.h, plan.h if plan is not None else None, _ptr(c0), _ptr(c1), c0.shape[0], primes,
                                    _ptr(out0), _ptr(out1), *tail, _stream_ptr()), sym)

    def _bsgs_call(self, sym, plan, c0, c1, out0, out1, workspace, primes, workspace_bytes):
        if workspace_bytes is None:
            workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
        self._plan_call(sym, plan, c0, c1, out0, out1, primes, (_ptr(workspace), workspace_bytes))

    def _mul_plain_sum(self, sym, in0, in1, pt, out0, out1, primes, ext):
        """The weighted sum over a stack; ext: of extended records, whose level is one below their rows and whose
        plaintexts have all np rows (no pt_primes argument)."""
        if primes is None:
            primes = in0.shape[2] - ext
        pt_rows = () if ext else (pt.shape[2],)
        _check(getattr(self.L, sym)(self.h, _ptr(in0), _ptr(in1), in0.shape[0], in0.shape[1], primes, _ptr(pt),
                                    pt.shape[0], *pt_rows, _ptr(out0), _ptr(out1), _stream_ptr()), sym)

    def ct_galois_many(self, c0, c1, elts, out0, out1, primes=None):
        """Hoisted rotations: out[e] = the rotation of the records (c0, c1) [B][primes][n] by elts[e], for all G
        elements from ONE digit decomposition of c1, with the installed Galois keys; out0, out1 are [G][B][primes][n].
        Decrypts like ct_galois per element, but is not bit-identical to it (the digits are those of c1, permuted after
        the transform)."""
        self._galois_set("se_amd_ct_galois_many_device", c0, c1, elts, out0, out1, primes)

    def ct_galois_sum(self, c0, c1, elts, out0, out1, add_input=False, primes=None):
        """The sum of the hoisted rotations by elts[0 .. G) in one record, plus the record itself with add_input:
        out0, out1 are [B][primes][n].  The transforms are those of one rotation whatever G is; an element listed twice
        counts twice."""
        self._galois_set("se_amd_ct_galois_sum_device", c0, c1, elts, out0, out1, primes,
                         flags=(1 if add_input else 0,))

    def lintrans_plan(self, elts, diag, diag0=None, pt_primes=None):
        """The plan of y = diag0 . x + sum_e diag[e] . rot_{elts[e]}(x): diag [G][pt_primes][n], diag0 [pt_primes][n] or
        None, device tensors in the layout encode_ntt writes.  Folds the diagonals into the installed Galois keys of
        `elts` (a snapshot; it synchronises) and returns an object with .close(); close it before the context."""
        return self._make_plan(LintransPlan, "se_amd_lintrans_create", (elts,), (diag, diag0),
                               diag.shape[1] if pt_primes is None else pt_primes)

    def ct_lintrans(self, plan, c0, c1, out0, out1, primes=None):
        """One launch: the plan's weighted sum of hoisted rotations of the records (c0, c1) [B][primes][n] ->
        (out0, out1) [B][primes][n]; the scale is multiplied by the diagonals' scale, the level is unchanged."""
        self._plan_call("se_amd_ct_lintrans_device", plan, c0, c1, out0, out1, primes)

    def ct_galois_sum_sp(self, c0, c1, elts, out0, out1, add_input=False, primes=None):
        """ct_galois_sum with the installed special-prime Galois keys on records (c0, c1) [B][primes][n], primes <=
        np - 1: the sum of the rotations by elts[0 .. G), plus the record itself with add_input, at the record's own
        scale from ONE decomposition and ONE division by the special prime.  One element without add_input gives the
        bits of ct_galois_sp; several carry one rounding instead of one each."""
        self._galois_set("se_amd_ct_galois_sum_sp_device", c0, c1, elts, out0, out1, primes,
                         flags=(1 if add_input else 0,))

    def lintrans_plan_sp(self, elts, diag, diag0=None, pt_primes=None):
        """lintrans_plan on the installed special-prime Galois keys: diag [G][np][n], diag0 [np][n] or None -- the
        diagonals need ALL np rows, the one at the special prime is folded into the key.  The plan serves ct_lintrans_sp
        at the levels 1 .. np - 1."""
        return self._make_plan(LintransPlan, "se_amd_lintrans_create_sp", (elts,), (diag, diag0),
                               diag.shape[1] if pt_primes is None else pt_primes)

    def ct_lintrans_sp(self, plan, c0, c1, out0, out1, primes=None):
        """One launch: the special-prime plan's weighted sum of rotations of the records (c0, c1) [B][primes][n],
        primes <= np - 1 -> (out0, out1) [B][primes][n]; the scale is multiplied by the diagonals' scale, the level is
        unchanged and no lift is needed."""
        self._plan_call("se_amd_ct_lintrans_sp_device", plan, c0, c1, out0, out1, primes)

    # ---- baby-step / giant-step linear transforms on the digit Galois keys
    def ct_mul_plain_sum(self, in0, pt, out0, in1=None, out1=None, primes=None):
        """Key-free weighted sum over a stack: in [E][B][primes][n] (one slab or two), pt [Gout][E][pt_primes][n] in
        encode_ntt's layout, out [Gout][B][primes][n]; out[g][b] = sum_e pt[g][e] . in[e][b] mod q_i, canonical.  Any
        32-bit plaintext word stands for its residue."""
        self._mul_plain_sum("se_amd_ct_mul_plain_sum_device", in0, in1, pt, out0, out1, primes, 0)

    def ct_galois_accum(self, in0, in1, elts, out0, out1, primes=None):
        """Rotate G different records and add: in [G][B][primes][n], out[b] = sum_g ct_galois(in[g][b], elts[g]) mod q_i
        with the installed Galois keys, [B][primes][n]; element 1 is the identity and needs no key.  Bit-identical to
        the modular sum of G ct_galois outputs."""
        self._galois_set("se_amd_ct_galois_accum_device", in0, in1, elts, out0, out1, primes, stacked=True)

    def bsgs_plan(self, baby, giant, diag, pt_primes=None):
        """The plan of y = sum_{g,b} diag[g][b] . rot_{giant[g] baby[b] mod 2n}(x): diag [n2][n1][pt_primes][n], a device
        tensor in the layout encode_ntt writes, the diagonal of the COMPOSITE element unrotated.  A snapshot of the
        diagonals only (it synchronises); keys are read at call time.  Returns an object with .close(); close it before
        the context."""
        return self._make_plan(BsgsPlan, "se_amd_bsgs_create", (baby, giant), (diag,),
                               diag.shape[2] if pt_primes is None else pt_primes)

    def bsgs_workspace_bytes(self, plan, records, primes):
        """Bytes of workspace ct_bsgs needs to take `records` records of level `primes` in one chunk."""
        return int(self.L.se_amd_bsgs_workspace_bytes(plan.h if plan is not None else None, records, primes))

    def ct_bsgs(self, plan, c0, c1, out0, out1, workspace, primes=None, workspace_bytes=None):
        """The plan's transform of the records (c0, c1) [B][primes][n] -> (out0, out1) [B][primes][n]: the many form for
        the baby steps, ct_mul_plain_sum, ct_galois_accum for the giant steps, in chunks of what `workspace` (a device
        tensor, 16-byte aligned) holds.  Every chunk size gives the same bits."""
        self._bsgs_call("se_amd_ct_bsgs_device", plan, c0, c1, out0, out1, workspace, primes, workspace_bytes)

    # ---- baby-step / giant-step linear transforms on the special-prime keys, division by P deferred
    def ct_galois_many_ext_sp(self, c0, c1, elts, out0, out1, primes=None):
        """The undivided baby steps: records (c0, c1) [B][L][n], L <= np - 1 -> extended records [G][B][L+1][n] (rows r <
        L modulo q_r, row L modulo the special prime), out[e] = P times the rotation by elts[e] plus its key-switch sum,
        from ONE decomposition of c1 under the installed special-prime keys.  Element 1 needs no key.  ct_mod_down_sp
        of out[e] is ct_galois_sp by elts[e]."""
        self._galois_set("se_amd_ct_galois_many_ext_sp_device", c0, c1, elts, out0, out1, primes)

    def ct_mul_plain_sum_ext_sp(self, in0, pt, out0, in1=None, out1=None, primes=None):
        """ct_mul_plain_sum on stacks of extended records: in [E][B][L+1][n], pt [Gout][E][np][n] (all np rows: row L of
        a record meets the plaintext's row at the special prime), out [Gout][B][L+1][n].  primes = L."""
        self._mul_plain_sum("se_amd_ct_mul_plain_sum_ext_sp_device", in0, in1, pt, out0, out1, primes, 1)

    def ct_mod_down_sp(self, in0, out0, in1=None, out1=None, primes=None, count=None):
        """The division by the special prime, rounded: extended records [..][L+1][n] (one slab or two) -> [..][L][n].
        count defaults to the product of the leading dimensions, primes = L to in0.shape[-2] - 1."""
        if primes is None:
            primes = in0.shape[-2] - 1
        if count is None:
            count = in0.numel() // (in0.shape[-2] * in0.shape[-1])
        _check(self.L.se_amd_ct_mod_down_sp_device(self.h, _ptr(in0), _ptr(in1), count, primes, _ptr(out0), _ptr(out1),
                                                   _stream_ptr()), "se_amd_ct_mod_down_sp_device")

    def ct_galois_accum_sp(self, in0, in1, elts, out0, out1, primes=None):
        """Rotate G different records under the special-prime keys and add, with ONE division by the special prime: in
        [G][B][L][n] -> [B][L][n].  Element 1 is the identity.  G = 1 has the bytes of ct_galois_sp; G >= 2 rounds once
        where G calls round G times."""
        self._galois_set("se_amd_ct_galois_accum_sp_device", in0, in1, elts, out0, out1, primes, stacked=True)

    def bsgs_plan_sp(self, baby, giant, diag, pt_primes=None):
        """bsgs_plan for ct_bsgs_sp: diag [n2][n1][np][n] with ALL np rows.  Diagonals only; the special-prime keys are
        read at call time.  The plan serves the levels 1 .. np - 1."""
        return self._make_plan(BsgsPlan, "se_amd_bsgs_create_sp", (baby, giant), (diag,),
                               diag.shape[2] if pt_primes is None else pt_primes)

    def ct_bsgs_sp(self, plan, c0, c1, out0, out1, workspace, primes=None, workspace_bytes=None):
        """The special-prime plan's transform of fresh records (c0, c1) [B][L][n], L <= np - 1 -> [B][L][n] at the
        record's scale times the diagonals': ct_galois_many_ext_sp, ct_mul_plain_sum_ext_sp, ct_mod_down_sp,
        ct_galois_accum_sp in chunks of what `workspace` holds.  Every chunk size gives the same bits."""
        self._bsgs_call("se_amd_ct_bsgs_sp_device", plan, c0, c1, out0, out1, workspace, primes, workspace_bytes)

    def prng_blocks(self, seeds, ctrs, out, outlen):
        _check(self.L.se_amd_prng_blocks_device(self.h, _ptr(seeds), _ptr(ctrs), _ptr(out), outlen,
                                                seeds.shape[0], _stream_ptr()),
               "se_amd_prng_blocks_device")

    def sample_uniform(self, seeds, out, ctr_in=None, ctr_out=None):
        _check(self.L.se_amd_sample_uniform_device(self.h, _ptr(seeds), _ptr(ctr_in),
                                                   seeds.shape[0], _ptr(out), _ptr(ctr_out),
                                                   _stream_ptr()), "se_amd_sample_uniform_device")

    def sample_ternary(self, seeds, codes, ctr_out=None):
        _check(self.L.se_amd_sample_ternary_device(self.h, _ptr(seeds), seeds.shape[0],
                                                   _ptr(codes), _ptr(ctr_out), _stream_ptr()),
               "se_amd_sample_ternary_device")

    def sample_cbd(self, seeds, out, blocks_per_ct, ctr_base=None):
        _check(self.L.se_amd_sample_cbd_device(self.h, _ptr(seeds), _ptr(ctr_base), seeds.shape[0],
                                               blocks_per_ct, _ptr(out), _stream_ptr()),
               "se_amd_sample_cbd_device")

    def word_ops(self, prime, op, a, b=None, c=None):
        """Device word arithmetic KAT hook: uint64 numpy operands in, uint32 numpy out."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).to(dev)
        ta, tb, tc = t(a), t(b), t(c)
        out = torch.zeros(ta.numel(), dtype=torch.int32, device=dev)
        _check(self.L.se_amd_word_ops_device(self.h, prime, op, _ptr(ta), _ptr(tb), _ptr(tc), _ptr(out),
                                             ta.numel(), _stream_ptr()), "se_amd_word_ops_device")
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)

    def pack_ternary(self, codes_np):
        import numpy as np
        codes = np.ascontiguousarray(codes_np, dtype=np.int8)
        out = np.zeros(codes.size // 4, dtype=np.uint8)
        self.L.se_amd_pack_ternary_host(_ptr(codes), codes.size, _ptr(out))
        return out

    # ---- host-pointer wrappers (numpy in / numpy out)
    def _host_out(self, out, B):
        """(c0, c1) host arrays: fresh, or the caller's (e.g. pinned) uint32[B][np][n] buffers."""
        import numpy as np
        if out is None:
            c0 = np.zeros((B, self.np, self.n), dtype=np.uint32)
            return c0, np.zeros_like(c0)
        c0, c1 = out
        for a in (c0, c1):
            if a.dtype != np.uint32 or a.shape != (B, self.np, self.n) or not a.flags.c_contiguous:
                raise ValueError("out buffers must be C-contiguous uint32[B][np][n]")
        return c0, c1

    def encrypt_sym_host(self, values, share_seeds, seeds, want_extra=False, out=None,
                         seed_compressed=False):
        import numpy as np
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, self.n // 2)
        B = v.shape[0]
        ss = np.ascontiguousarray(share_seeds, dtype=np.uint8).reshape(B, 64)
        sd = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(B, 64)
        c0, c1 = self._host_out(out, B)
        if seed_compressed:
            c1 = None                  # only c0 crosses PCIe; c1 = expand_c1(share_seeds)
        ntt_pte = np.zeros_like(c0) if want_extra else None
        pte = np.zeros((B, self.n), dtype=np.int64) if want_extra else None
        status = np.zeros(B, dtype=np.uint8)
        rc = _check(self.L.se_amd_encrypt_sym_host(self.h, _ptr(v), B, _ptr(ss), _ptr(sd),
                                                   _ptr(c0), _ptr(c1), _ptr(ntt_pte), _ptr(pte),
                                                   _ptr(status)), "se_amd_encrypt_sym_host")
        return dict(failed=rc, c0=c0, c1=c1, ntt_pte=ntt_pte, pte=pte, status=status)

    def encrypt_asym_host(self, values, seeds, want_extra=False, out=None):
        import numpy as np
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, self.n // 2)
        B = v.shape[0]
        sd = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(B, 64)
        c0, c1 = self._host_out(out, B)
        ntt_pte = np.zeros_like(c0) if want_extra else None
        pte = np.zeros((B, self.n), dtype=np.int64) if want_extra else None
        status = np.zeros(B, dtype=np.uint8)
        rc = _check(self.L.se_amd_encrypt_asym_host(self.h, _ptr(v), B, _ptr(sd), _ptr(c0),
                                                    _ptr(c1), _ptr(ntt_pte), _ptr(pte),
                                                    _ptr(status)), "se_amd_encrypt_asym_host")
        return dict(failed=rc, c0=c0, c1=c1, ntt_pte=ntt_pte, pte=pte, status=status)

    # ---- profiling
    def set_profiling(self, on=True):
        _check(self.L.se_amd_set_profiling(self.h, 1 if on else 0), "se_amd_set_profiling")

    def stage_ms(self, reset=True):
        """{stage: (total_ms, launches)} measured with HIP events on the launch stream."""
        ms = (C.c_float * len(STAGES))()
        cnt = (C.c_uint64 * len(STAGES))()
        _check(self.L.se_amd_stage_ms(self.h, ms, cnt, 1 if reset else 0), "se_amd_stage_ms")
        return {s: (float(ms[i]), int(cnt[i])) for i, s in enumerate(STAGES)}

    def set_pipeline(self, overlap=True, split=True):
        _check(self.L.se_amd_set_pipeline(self.h, int(overlap), int(split)), "se_amd_set_pipeline")

    def set_asym_chunks(self, chunks):
        _check(self.L.se_amd_set_asym_chunks(self.h, chunks), "se_amd_set_asym_chunks")

    def set_debug_flags(self, flags):
        _check(self.L.se_amd_set_debug_flags(self.h, flags), "se_amd_set_debug_flags")

    def set_speculation_capacity(self, cap):
        _check(self.L.se_amd_set_speculation_capacity(self.h, cap),
               "se_amd_set_speculation_capacity")

    def set_host_chunk(self, cts):
        _check(self.L.se_amd_set_host_chunk(self.h, cts), "se_amd_set_host_chunk")

    def reserve(self, B):
        _check(self.L.se_amd_reserve(self.h, B), "se_amd_reserve")

    def set_reject_list_capacity(self, cap):
        _check(self.L.se_amd_set_reject_list_capacity(self.h, cap),
               "se_amd_set_reject_list_capacity")
