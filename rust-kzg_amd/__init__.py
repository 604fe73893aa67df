"""rust-kzg_amd — MI355X-native KZG hot path (MSM + NTT) behind rust-kzg's own seams.

This package is host-side plumbing only: it loads the C-ABI library
(csrc/libkzg_mi355x.so, built by build.py with hipcc for gfx950) and mirrors the
reference's plug-in interface for the path:

  prepare_multi_scalar_mult / multi_scalar_mult_prepared / multi_scalar_mult
      = blst-sppark/src/lib.rs:8-62 (the three FFI wrappers `rust-kzg-blst` calls)
  FFTSettings.fft_fr / das_fft_extension / fft_g1
      = kzg::FFTFr / kzg::DASExtension / kzg::FFTG1 for FsFFTSettings (blst/src/fft_fr.rs:156-165,
        blst/src/data_availability_sampling.rs:78-100, blst/src/fft_g1.rs:54-83)

There is no CPU fallback: if the library is missing or no GPU is visible the calls raise.
The directory name contains a hyphen; import it with `load()` from __graft_entry__ /
tests (importlib under the module name `rust_kzg_amd`).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KZGAMD_LIB") or os.path.join(HERE, "csrc", "libkzg_mi355x.so")  # KZGAMD_LIB: A/B builds


class KzgAmdError(RuntimeError):
    pass


class RustError(C.Structure):
    _fields_ = [("code", C.c_int), ("message", C.c_char_p)]


class BlstFr(C.Structure):
    _fields_ = [("l", C.c_uint64 * 4)]


class BlstFp(C.Structure):
    _fields_ = [("l", C.c_uint64 * 6)]


class BlstP1Affine(C.Structure):
    _fields_ = [("x", BlstFp), ("y", BlstFp)]


class BlstP1(C.Structure):
    _fields_ = [("x", BlstFp), ("y", BlstFp), ("z", BlstFp)]


class BlstFp2(C.Structure):
    _fields_ = [("fp", BlstFp * 2)]


class BlstP2(C.Structure):
    _fields_ = [("x", BlstFp2), ("y", BlstFp2), ("z", BlstFp2)]


_lib = None

# every symbol include/kzg_mi355x.h declares; tests check the library exports all of them
EXPORTS = [
    "kzgamd_config_init", "kzgamd_tuning_keys", "kzgamd_msm_attach_matrix", "kzgamd_msm_matrix_shape", "kzgamd_pin_host_buffer", "kzgamd_unpin_host_buffer", "kzgamd_prepare_msm_ex", "kzgamd_prepare_msm_matrix", "kzgamd_mult_pippenger_matrix",
    "kzgamd_msm_create_device_ex", "kzgamd_ntt_new_ex", "kzgamd_load_trusted_setup_ex", "kzgamd_load_trusted_setup_file_ex",
    "kzgamd_load_trusted_setup_file_multi_ex",
    "prepare_msm", "mult_pippenger_prepared", "mult_pippenger", "free_msm", "mult_pippenger_prepared_batch",
    "kzgamd_msm_prepared_batch_device", "kzgamd_msm_info", "kzgamd_msm_uses_wide_table", "kzgamd_msm_set_profile", "kzgamd_msm_get_profile",
    "kzgamd_device_count", "kzgamd_version", "kzgamd_msm_create_device", "kzgamd_generate_points",
    "kzgamd_ntt_new", "kzgamd_ntt_free", "ntt_fr", "das_fft_extension", "kzgamd_ntt_fr_device", "kzgamd_ntt_roots", "kzgamd_ntt_plan_dump", "kzgamd_ntt_das_plan_dump", "kzgamd_das_fft_extension_device",
    "fft_g1", "kzgamd_fft_g1_batch", "kzgamd_g1_sum",
    "kzgamd_fk20_new", "kzgamd_fk20_free", "kzgamd_fk20_da", "kzgamd_fk20_info",
    "kzgamd_kzg_new", "kzgamd_kzg_free", "kzgamd_kzg_info", "kzgamd_kzg_commit", "kzgamd_kzg_open", "kzgamd_kzg_check",
    "kzgamd_kzg_check_batch", "kzgamd_kzg_check_batch_g1", "kzgamd_kzg_batch_challenge",
    "kzgamd_poly_new", "kzgamd_poly_free", "kzgamd_poly_info", "kzgamd_poly_eval", "kzgamd_poly_scale", "kzgamd_poly_mul",
    "kzgamd_poly_inverse", "kzgamd_poly_div", "kzgamd_poly_transform_len",
    "kzgamd_poly_zero_partial", "kzgamd_poly_reduce_partials", "kzgamd_poly_zero_poly", "kzgamd_poly_recover",
    "kzgamd_poly_zero_info", "kzgamd_poly_zero_plan",
    "load_trusted_setup", "load_trusted_setup_file", "free_trusted_setup", "blob_to_kzg_commitment",
    "compute_kzg_proof", "compute_blob_kzg_proof", "kzgamd_compute_blob_kzg_proof_batch", "compute_challenge",
    "bytes_to_kzg_commitment", "bytes_from_bls_field", "compute_cells_and_kzg_proofs",
    "recover_cells_and_kzg_proofs", "verify_cell_kzg_proof_batch", "compute_verify_cell_kzg_proof_batch_challenge",
    "kzgamd_recover_cells_and_kzg_proofs_batch",
    "kzgamd_verify_cell_kzg_proof_batch_many", "kzgamd_verify_cell_kzg_proof_batch_many_g1", "kzgamd_vcells_info",
    "kzgamd_vcells_timing",
    "kzgamd_compute_cells_and_kzg_proofs_batch", "kzgamd_compute_challenges_and_evaluate_batch",
    "kzgamd_blob_to_kzg_commitment_batch", "kzgamd_blob_to_kzg_commitment_device", "kzgamd_settings_msm_handle",
    "kzgamd_msm_reserve", "kzgamd_msm_device", "kzgamd_set_device", "kzgamd_get_device", "kzgamd_settings_device",
    "kzgamd_settings_reserve", "kzgamd_settings_table_info", "kzgamd_verify_kzg_proof_batch_g1", "kzgamd_verify_blob_kzg_proof_batch_g1",
    "verify_kzg_proof", "verify_blob_kzg_proof", "verify_blob_kzg_proof_batch", "kzgamd_pairings_verify",
    "kzgamd_pairings_verify_batch", "kzgamd_pairing_info",
    "kzgamd_compute_blob_kzg_proof_device",
    "kzgamd_p2_uncompress", "kzgamd_p2_compress", "kzgamd_p2_generator", "kzgamd_p2_mult", "kzgamd_p2_add",
    "kzgamd_g1_mul_batch", "kzgamd_g2_mul_batch", "kzgamd_generate_trusted_setup", "kzgamd_group_mul_info",
    "kzgamd_g1_compress_batch", "kzgamd_g1_to_affine_batch", "kzgamd_g1_uncompress_batch", "kzgamd_g2_compress_batch",
    "kzgamd_g2_uncompress_batch", "kzgamd_p2_in_g2", "kzgamd_codec_info",
    "kzgamd_write_trusted_setup_file", "kzgamd_read_trusted_setup_file",
    "kzgamd_g2_lincomb", "kzgamd_g2_lincomb_info", "kzgamd_verify_trusted_setup", "kzgamd_verify_trusted_setup_file",
    "kzgamd_g2_msm_new", "kzgamd_g2_msm_free", "kzgamd_g2_msm", "kzgamd_g2_msm_info",
    "kzgamd_load_trusted_setup_file_multi", "kzgamd_free_trusted_setup_multi", "kzgamd_blob_to_kzg_commitment_batch_multi",
    "kzgamd_compute_blob_kzg_proof_batch_multi", "kzgamd_compute_cells_and_kzg_proofs_batch_multi",
    "kzgamd_verify_blob_kzg_proof_batch_multi", "kzgamd_mult_pippenger_prepared_multi", "kzgamd_shard_range",
]


class CKZGSettings(C.Structure):
    """kzg/src/eth/c_bindings.rs:55-108"""
    _fields_ = [("roots_of_unity", C.c_void_p), ("brp_roots_of_unity", C.c_void_p),
                ("reverse_roots_of_unity", C.c_void_p), ("g1_values_monomial", C.c_void_p),
                ("g1_values_lagrange_brp", C.c_void_p), ("g2_values_monomial", C.c_void_p),
                ("x_ext_fft_columns", C.c_void_p), ("tables", C.c_void_p), ("wbits", C.c_size_t),
                ("scratch_size", C.c_size_t)]


C_KZG_OK, C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC = 0, 1, 2, 3
BYTES_PER_BLOB = 131072


class KzgAmdConfig(C.Structure):
    """include/kzg_mi355x.h: the configuration every creating entry point's _ex form takes"""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("table_budget_bytes", C.c_uint64), ("tuning", C.c_char_p)]


NO_TABLES = (1 << 64) - 1


def make_config(device=-1, table_budget_gb=None, tuning=None, no_tables=False):
    """KzgAmdConfig for the `config=` arguments below.  table_budget_gb: HBM each fixed-base table may take (None = the
    library's default); tuning: a dict or "key=value;key=value" string of the measured switches (tuning_keys())."""
    cfg = KzgAmdConfig()
    lib().kzgamd_config_init(C.byref(cfg))
    cfg.device = device
    if no_tables:
        cfg.table_budget_bytes = NO_TABLES
    elif table_budget_gb is not None:
        cfg.table_budget_bytes = max(1, int(table_budget_gb * 1e9))
    if isinstance(tuning, dict):
        tuning = ";".join("%s=%d" % (k, int(v)) for k, v in tuning.items())
    if tuning:
        cfg.tuning = tuning.encode()
    return cfg


def _cfgp(config):
    return C.byref(config) if config is not None else None


def tuning_keys():
    """{name: (default, lo, hi, meaning)} — the table of rust-kzg_amd/csrc/config.h"""
    out = {}
    for line in lib().kzgamd_tuning_keys().decode().splitlines():
        name, d, lo, hi, what = line.split(" ", 4)
        out[name] = (int(d), int(lo), int(hi), what)
    return out


def lib():
    """Load libkzg_mi355x.so; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KzgAmdError("libkzg_mi355x.so is not built (%s); run __graft_entry__.build()" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    L.prepare_msm.restype = vp
    L.prepare_msm.argtypes = [vp, sz]
    cp = C.POINTER(KzgAmdConfig)
    L.kzgamd_config_init.restype = None
    L.kzgamd_config_init.argtypes = [cp]
    L.kzgamd_tuning_keys.restype = C.c_char_p
    L.kzgamd_prepare_msm_ex.restype = vp
    L.kzgamd_prepare_msm_ex.argtypes = [vp, sz, cp]
    L.kzgamd_prepare_msm_matrix.restype = vp
    L.kzgamd_prepare_msm_matrix.argtypes = [vp, sz, sz, cp]
    L.kzgamd_pin_host_buffer.restype = C.c_int
    L.kzgamd_pin_host_buffer.argtypes = [vp, sz]
    L.kzgamd_unpin_host_buffer.restype = C.c_int
    L.kzgamd_unpin_host_buffer.argtypes = [vp]
    L.kzgamd_msm_matrix_shape.restype = C.c_int
    L.kzgamd_msm_matrix_shape.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.kzgamd_msm_attach_matrix.restype = RustError
    L.kzgamd_msm_attach_matrix.argtypes = [vp, vp, sz, sz, cp]
    L.kzgamd_mult_pippenger_matrix.restype = RustError
    L.kzgamd_mult_pippenger_matrix.argtypes = [vp, vp, vp, sz]
    L.kzgamd_msm_create_device_ex.restype = vp
    L.kzgamd_msm_create_device_ex.argtypes = [vp, sz, C.c_int, cp]
    L.kzgamd_ntt_new_ex.restype = vp
    L.kzgamd_ntt_new_ex.argtypes = [C.c_uint, cp]
    L.free_msm.restype = None
    L.free_msm.argtypes = [vp]
    L.mult_pippenger_prepared.restype = RustError
    L.mult_pippenger_prepared.argtypes = [vp, vp, sz, vp]
    L.mult_pippenger_prepared_batch.restype = RustError
    L.mult_pippenger_prepared_batch.argtypes = [vp, vp, sz, sz, vp]
    L.mult_pippenger.restype = RustError
    L.mult_pippenger.argtypes = [vp, vp, sz, vp]
    L.kzgamd_msm_prepared_batch_device.restype = RustError
    L.kzgamd_msm_prepared_batch_device.argtypes = [vp, vp, vp, sz, sz, C.c_int, vp]
    L.kzgamd_msm_info.restype = C.c_int
    L.kzgamd_msm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(sz), C.POINTER(sz)]
    L.kzgamd_msm_uses_wide_table.restype = C.c_int
    L.kzgamd_msm_uses_wide_table.argtypes = [vp]
    L.kzgamd_device_count.restype = C.c_int
    L.kzgamd_version.restype = C.c_char_p
    L.kzgamd_msm_set_profile.restype = C.c_int
    L.kzgamd_msm_set_profile.argtypes = [vp, C.c_int]
    L.kzgamd_msm_get_profile.restype = C.c_int
    L.kzgamd_msm_get_profile.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.kzgamd_msm_create_device.restype = vp
    L.kzgamd_msm_create_device.argtypes = [vp, sz, C.c_int]
    L.kzgamd_generate_points.restype = RustError
    L.kzgamd_generate_points.argtypes = [vp, sz, C.c_uint64, vp]
    L.kzgamd_ntt_new.restype = vp
    L.kzgamd_ntt_new.argtypes = [C.c_uint]
    L.kzgamd_ntt_free.restype = None
    L.kzgamd_ntt_free.argtypes = [vp]
    L.ntt_fr.restype = C.c_int
    L.ntt_fr.argtypes = [vp, vp, vp, sz, C.c_int]
    L.das_fft_extension.restype = C.c_int
    L.das_fft_extension.argtypes = [vp, vp, vp, sz]
    L.kzgamd_ntt_fr_device.restype = C.c_int
    L.kzgamd_ntt_fr_device.argtypes = [vp, vp, vp, sz, sz, C.c_int, vp]
    L.kzgamd_das_fft_extension_device.restype = C.c_int
    L.kzgamd_das_fft_extension_device.argtypes = [vp, vp, vp, vp, sz, sz, vp]
    L.kzgamd_g1_sum.restype = None
    L.kzgamd_g1_sum.argtypes = [vp, vp, sz]
    L.fft_g1.restype = C.c_int
    L.fft_g1.argtypes = [vp, vp, vp, sz, C.c_int]
    L.kzgamd_fft_g1_batch.restype = C.c_int
    L.kzgamd_fft_g1_batch.argtypes = [vp, vp, vp, sz, sz, C.c_int]
    L.kzgamd_fk20_new.restype = vp
    L.kzgamd_fk20_new.argtypes = [vp, vp, sz, sz, sz, cp, C.POINTER(C.c_int)]
    L.kzgamd_fk20_free.restype = None
    L.kzgamd_fk20_free.argtypes = [vp]
    L.kzgamd_fk20_da.restype = C.c_int
    L.kzgamd_fk20_da.argtypes = [vp, vp, vp, sz, sz, C.c_int]
    L.kzgamd_fk20_info.restype = C.c_int
    L.kzgamd_fk20_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_int)]
    L.kzgamd_kzg_new.restype = vp
    L.kzgamd_kzg_new.argtypes = [vp, vp, sz, vp, sz, cp, C.POINTER(C.c_int)]
    L.kzgamd_kzg_free.restype = None
    L.kzgamd_kzg_free.argtypes = [vp]
    L.kzgamd_kzg_info.restype = C.c_int
    L.kzgamd_kzg_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.kzgamd_kzg_commit.restype = C.c_int
    L.kzgamd_kzg_commit.argtypes = [vp, vp, vp, sz, sz]
    L.kzgamd_kzg_open.restype = C.c_int
    L.kzgamd_kzg_open.argtypes = [vp, vp, vp, vp, sz, sz, vp, sz, sz]
    L.kzgamd_kzg_check.restype = C.c_int
    L.kzgamd_kzg_check.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz]
    L.kzgamd_kzg_check_batch.restype = C.c_int
    L.kzgamd_kzg_check_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, vp]
    L.kzgamd_kzg_check_batch_g1.restype = C.c_int
    L.kzgamd_kzg_check_batch_g1.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, vp]
    L.kzgamd_kzg_batch_challenge.restype = C.c_int
    L.kzgamd_kzg_batch_challenge.argtypes = [vp, vp, vp, vp, vp, sz, sz]
    L.kzgamd_poly_new.restype = vp
    L.kzgamd_poly_new.argtypes = [vp, cp, C.POINTER(C.c_int)]
    L.kzgamd_poly_free.restype = None
    L.kzgamd_poly_free.argtypes = [vp]
    L.kzgamd_poly_info.restype = C.c_int
    L.kzgamd_poly_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.kzgamd_poly_eval.restype = C.c_int
    L.kzgamd_poly_eval.argtypes = [vp, vp, vp, sz, sz, vp, sz]
    L.kzgamd_poly_scale.restype = C.c_int
    L.kzgamd_poly_scale.argtypes = [vp, vp, vp, sz, sz, C.c_int]
    L.kzgamd_poly_mul.restype = C.c_int
    L.kzgamd_poly_mul.argtypes = [vp, vp, vp, sz, vp, sz, sz, sz, C.c_int]
    L.kzgamd_poly_inverse.restype = C.c_int
    L.kzgamd_poly_inverse.argtypes = [vp, vp, vp, sz, sz, sz]
    L.kzgamd_poly_div.restype = C.c_int
    L.kzgamd_poly_div.argtypes = [vp, vp, vp, sz, vp, sz, sz]
    L.kzgamd_poly_transform_len.restype = sz
    L.kzgamd_poly_transform_len.argtypes = [C.c_int, sz, sz, sz]
    L.kzgamd_poly_zero_partial.restype = C.c_int
    L.kzgamd_poly_zero_partial.argtypes = [vp, vp, C.POINTER(C.c_uint64), sz, sz]
    L.kzgamd_poly_reduce_partials.restype = C.c_int
    L.kzgamd_poly_reduce_partials.argtypes = [vp, vp, sz, vp, C.POINTER(sz), sz]
    L.kzgamd_poly_zero_poly.restype = C.c_int
    L.kzgamd_poly_zero_poly.argtypes = [vp, vp, vp, sz, C.POINTER(C.c_uint64), C.POINTER(sz), sz, C.c_int]
    L.kzgamd_poly_recover.restype = C.c_int
    L.kzgamd_poly_recover.argtypes = [vp, vp, vp, C.POINTER(C.c_uint8), sz, sz, C.c_int]
    L.kzgamd_poly_zero_info.restype = C.c_int
    L.kzgamd_poly_zero_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.kzgamd_poly_zero_plan.restype = sz
    L.kzgamd_poly_zero_plan.argtypes = [sz, C.POINTER(sz)]
    L.kzgamd_ntt_roots.restype = C.c_int
    L.kzgamd_ntt_roots.argtypes = [vp, vp, vp, vp]
    sp = C.POINTER(CKZGSettings)
    L.load_trusted_setup.restype = C.c_int
    L.load_trusted_setup.argtypes = [sp, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64,
                                     C.c_uint64]
    L.load_trusted_setup_file.restype = C.c_int
    L.load_trusted_setup_file.argtypes = [sp, vp]
    L.kzgamd_load_trusted_setup_ex.restype = C.c_int
    L.kzgamd_load_trusted_setup_ex.argtypes = [sp, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64,
                                               C.c_uint64, cp]
    L.kzgamd_load_trusted_setup_file_ex.restype = C.c_int
    L.kzgamd_load_trusted_setup_file_ex.argtypes = [sp, vp, cp]
    L.kzgamd_load_trusted_setup_file_multi_ex.restype = C.c_int
    L.kzgamd_load_trusted_setup_file_multi_ex.argtypes = [vp, vp, sz, vp, cp]
    L.free_trusted_setup.restype = None
    L.free_trusted_setup.argtypes = [sp]
    L.kzgamd_compute_challenges_and_evaluate_batch.restype = C.c_int
    L.kzgamd_compute_challenges_and_evaluate_batch.argtypes = [vp, vp, vp, vp, sz, sp]
    L.blob_to_kzg_commitment.restype = C.c_int
    L.blob_to_kzg_commitment.argtypes = [vp, vp, sp]
    L.kzgamd_blob_to_kzg_commitment_batch.restype = C.c_int
    L.kzgamd_blob_to_kzg_commitment_batch.argtypes = [vp, vp, sz, sp]
    L.kzgamd_blob_to_kzg_commitment_device.restype = C.c_int
    L.kzgamd_blob_to_kzg_commitment_device.argtypes = [vp, vp, vp, vp, sz, sp, vp]
    L.compute_kzg_proof.restype = C.c_int
    L.compute_kzg_proof.argtypes = [vp, vp, vp, vp, sp]
    L.compute_blob_kzg_proof.restype = C.c_int
    L.compute_blob_kzg_proof.argtypes = [vp, vp, vp, sp]
    L.kzgamd_compute_blob_kzg_proof_device.restype = C.c_int
    L.kzgamd_compute_blob_kzg_proof_device.argtypes = [vp, vp, vp, vp, vp, sz, sp, vp]
    L.kzgamd_compute_blob_kzg_proof_batch.restype = C.c_int
    L.kzgamd_compute_blob_kzg_proof_batch.argtypes = [vp, vp, vp, sz, sp]
    L.compute_challenge.restype = None
    L.compute_challenge.argtypes = [vp, vp, vp]
    L.bytes_to_kzg_commitment.restype = C.c_int
    L.bytes_to_kzg_commitment.argtypes = [vp, vp]
    L.bytes_from_bls_field.restype = None
    L.bytes_from_bls_field.argtypes = [vp, vp]
    L.compute_cells_and_kzg_proofs.restype = C.c_int
    L.compute_cells_and_kzg_proofs.argtypes = [vp, vp, vp, sp]
    L.kzgamd_compute_cells_and_kzg_proofs_batch.restype = C.c_int
    L.kzgamd_compute_cells_and_kzg_proofs_batch.argtypes = [vp, vp, vp, sz, sp]
    L.kzgamd_recover_cells_and_kzg_proofs_batch.argtypes = [vp, vp, vp, vp, vp, sz, sp]
    L.kzgamd_verify_cell_kzg_proof_batch_many.restype = C.c_int
    L.kzgamd_verify_cell_kzg_proof_batch_many.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, vp, sp]
    L.kzgamd_verify_cell_kzg_proof_batch_many_g1.restype = C.c_int
    L.kzgamd_verify_cell_kzg_proof_batch_many_g1.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, sp]
    L.kzgamd_vcells_info.restype = C.c_int
    L.kzgamd_vcells_info.argtypes = [vp]
    L.kzgamd_vcells_timing.restype = C.c_int
    L.kzgamd_vcells_timing.argtypes = [sp, vp]
    L.kzgamd_settings_msm_handle.restype = vp
    L.kzgamd_settings_msm_handle.argtypes = [sp]
    L.kzgamd_msm_reserve.restype = RustError
    L.kzgamd_msm_reserve.argtypes = [vp, sz, sz, vp]
    L.kzgamd_msm_device.restype = C.c_int
    L.kzgamd_msm_device.argtypes = [vp]
    L.kzgamd_set_device.restype = C.c_int
    L.kzgamd_set_device.argtypes = [C.c_int]
    L.kzgamd_get_device.restype = C.c_int
    L.kzgamd_settings_device.restype = C.c_int
    L.kzgamd_settings_device.argtypes = [sp]
    L.kzgamd_settings_reserve.restype = C.c_int
    L.kzgamd_settings_reserve.argtypes = [sp, sz, vp]
    L.kzgamd_verify_kzg_proof_batch_g1.restype = C.c_int
    L.kzgamd_verify_kzg_proof_batch_g1.argtypes = [vp, vp, vp, vp, vp, vp, sz, sp]
    L.kzgamd_verify_blob_kzg_proof_batch_g1.restype = C.c_int
    L.kzgamd_verify_blob_kzg_proof_batch_g1.argtypes = [vp, vp, vp, vp, vp, sz, sp]
    bp = C.POINTER(C.c_bool)
    L.verify_kzg_proof.restype = C.c_int
    L.verify_kzg_proof.argtypes = [bp, vp, vp, vp, vp, sp]
    L.verify_blob_kzg_proof.restype = C.c_int
    L.verify_blob_kzg_proof.argtypes = [bp, vp, vp, vp, sp]
    L.verify_blob_kzg_proof_batch.restype = C.c_int
    L.verify_blob_kzg_proof_batch.argtypes = [bp, vp, vp, vp, sz, sp]
    L.kzgamd_pairings_verify.restype = C.c_int
    L.kzgamd_pairings_verify.argtypes = [vp, vp, vp, vp]
    L.kzgamd_pairings_verify_batch.restype = C.c_int
    L.kzgamd_pairings_verify_batch.argtypes = [vp, vp, vp, vp, vp, C.c_size_t]
    L.kzgamd_pairing_info.restype = C.c_int
    L.kzgamd_pairing_info.argtypes = [vp]
    L.kzgamd_p2_uncompress.restype = C.c_int
    L.kzgamd_p2_uncompress.argtypes = [vp, vp]
    L.kzgamd_p2_compress.restype = None
    L.kzgamd_p2_compress.argtypes = [vp, vp]
    L.kzgamd_p2_generator.restype = None
    L.kzgamd_p2_generator.argtypes = [vp]
    L.kzgamd_p2_mult.restype = None
    L.kzgamd_p2_mult.argtypes = [vp, vp, vp]
    L.kzgamd_p2_add.restype = None
    L.kzgamd_p2_add.argtypes = [vp, vp, vp]
    L.kzgamd_g1_mul_batch.restype = C.c_int
    L.kzgamd_g1_mul_batch.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.kzgamd_g2_mul_batch.restype = C.c_int
    L.kzgamd_g2_mul_batch.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.kzgamd_generate_trusted_setup.restype = C.c_int
    L.kzgamd_generate_trusted_setup.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp]
    L.kzgamd_group_mul_info.restype = C.c_int
    L.kzgamd_group_mul_info.argtypes = [vp, vp, vp]
    for name in ("kzgamd_g1_compress_batch", "kzgamd_g1_to_affine_batch", "kzgamd_g2_compress_batch"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, vp, C.c_size_t, vp]
    for name in ("kzgamd_g1_uncompress_batch", "kzgamd_g2_uncompress_batch"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp]
    L.kzgamd_p2_in_g2.restype = C.c_int
    L.kzgamd_p2_in_g2.argtypes = [vp]
    L.kzgamd_codec_info.restype = C.c_int
    L.kzgamd_codec_info.argtypes = [vp]
    L.kzgamd_write_trusted_setup_file.restype = C.c_int
    L.kzgamd_write_trusted_setup_file.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    L.kzgamd_read_trusted_setup_file.restype = C.c_int
    L.kzgamd_read_trusted_setup_file.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.kzgamd_g2_lincomb.restype = C.c_int
    L.kzgamd_g2_lincomb.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.kzgamd_g2_lincomb_info.restype = C.c_int
    L.kzgamd_g2_lincomb_info.argtypes = [vp]
    L.kzgamd_g2_msm_new.restype = vp
    L.kzgamd_g2_msm_new.argtypes = [vp, C.c_size_t, vp, C.POINTER(C.c_int)]
    L.kzgamd_g2_msm_free.restype = None
    L.kzgamd_g2_msm_free.argtypes = [vp]
    L.kzgamd_g2_msm.restype = C.c_int
    L.kzgamd_g2_msm.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t]
    L.kzgamd_g2_msm_info.restype = C.c_int
    L.kzgamd_g2_msm_info.argtypes = [vp, vp, vp, vp, vp, vp]
    L.kzgamd_verify_trusted_setup.restype = C.c_int
    L.kzgamd_verify_trusted_setup.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp]
    L.kzgamd_verify_trusted_setup_file.restype = C.c_int
    L.kzgamd_verify_trusted_setup_file.argtypes = [vp, vp, vp, vp, vp]
    L.kzgamd_load_trusted_setup_file_multi.restype = C.c_int
    L.kzgamd_load_trusted_setup_file_multi.argtypes = [vp, vp, sz, vp]
    L.kzgamd_free_trusted_setup_multi.restype = None
    L.kzgamd_free_trusted_setup_multi.argtypes = [vp, sz]
    L.kzgamd_blob_to_kzg_commitment_batch_multi.restype = C.c_int
    L.kzgamd_blob_to_kzg_commitment_batch_multi.argtypes = [vp, vp, sz, vp, sz]
    L.kzgamd_compute_blob_kzg_proof_batch_multi.restype = C.c_int
    L.kzgamd_compute_blob_kzg_proof_batch_multi.argtypes = [vp, vp, vp, sz, vp, sz]
    L.kzgamd_compute_cells_and_kzg_proofs_batch_multi.restype = C.c_int
    L.kzgamd_compute_cells_and_kzg_proofs_batch_multi.argtypes = [vp, vp, vp, sz, vp, sz]
    L.kzgamd_verify_blob_kzg_proof_batch_multi.restype = C.c_int
    L.kzgamd_verify_blob_kzg_proof_batch_multi.argtypes = [bp, vp, vp, vp, sz, vp, sz]
    L.kzgamd_shard_range.restype = C.c_int
    L.kzgamd_shard_range.argtypes = [sz, sz, sz, C.POINTER(sz), C.POINTER(sz)]
    L.kzgamd_mult_pippenger_prepared_multi.restype = RustError
    L.kzgamd_mult_pippenger_prepared_multi.argtypes = [vp, sz, vp, vp, vp]
    _lib = L
    return L


def _check(err, what):
    if err.code != 0:
        msg = err.message.decode() if err.message else "error %d" % err.code
        raise KzgAmdError("%s: %s" % (what, msg))


def _addr(buf):
    return C.cast(buf, C.c_void_p) if not isinstance(buf, int) else C.c_void_p(buf)


class PreparedMsm:
    """Owning handle = the reference's SpparkPrecomputation.table (kzg/src/msm/sppark.rs:5-22)."""

    def __init__(self, points, npoints, config=None):
        self.npoints = npoints
        self.handle = lib().kzgamd_prepare_msm_ex(_addr(points), npoints, _cfgp(config)) if config is not None \
            else lib().prepare_msm(_addr(points), npoints)
        if not self.handle:
            raise KzgAmdError("prepare_msm failed (no GPU, or bad arguments)")

    def attach_matrix(self, points, rows, cols, config=None):
        """kzgamd_msm_attach_matrix: this handle also answers multiply_batch (the reference's precompute(points, matrix))"""
        _check(lib().kzgamd_msm_attach_matrix(self.handle, _addr(points), rows, cols, _cfgp(config)), "kzgamd_msm_attach_matrix")
        self.rows, self.cols = rows, cols

    def multiply_batch(self, scalars, nmat=1):
        """scalars: blst_fr[nmat * rows * cols] (Montgomery) -> (BlstP1 * (nmat * rows)); needs a matrix (attach_matrix / MatrixMsm)"""
        out = (BlstP1 * (nmat * self.rows))()
        _check(lib().kzgamd_mult_pippenger_matrix(self.handle, out, _addr(scalars), nmat), "kzgamd_mult_pippenger_matrix")
        return out

    def info(self):
        c, rows, nb, n = C.c_int(), C.c_int(), C.c_size_t(), C.c_size_t()
        lib().kzgamd_msm_info(self.handle, C.byref(c), C.byref(rows), C.byref(nb), C.byref(n))
        wide = lib().kzgamd_msm_uses_wide_table(self.handle)
        return {"window_bits": c.value, "rows": rows.value, "nbuckets": nb.value, "npoints": n.value,
                "wide_table": bool(wide), "wide_glv": wide == 2,
                "adds_per_scalar": rows.value * (2 if wide == 2 else 1)}

    def close(self):
        if self.handle:
            lib().free_msm(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prepare_multi_scalar_mult(points, npoints, config=None):
    """blst-sppark/src/lib.rs:8-17.  points: ctypes array / buffer of blst_p1_affine."""
    return PreparedMsm(points, npoints, config)


class MatrixMsm(PreparedMsm):
    """rows base sets of cols points in one table: the precomputation behind G1LinComb::g1_lincomb_batch
    (kzg/src/lib.rs:156-181 -> BgmwTable::multiply_batch, kzg/src/msm/bgmw.rs:306-380).  points[r * cols + c]."""

    def __init__(self, points, rows, cols, config=None):
        self.rows, self.cols, self.npoints = rows, cols, rows * cols
        self.handle = lib().kzgamd_prepare_msm_matrix(_addr(points), rows, cols, _cfgp(config))
        if not self.handle:
            raise KzgAmdError("kzgamd_prepare_msm_matrix failed (no GPU, bad arguments, or no wide table fits the budget)")



def multi_scalar_mult_prepared(msm, scalars, npoints):
    """blst-sppark/src/lib.rs:19-38.  scalars: blst_fr[npoints] (Montgomery).  Returns BlstP1."""
    out = BlstP1()
    _check(lib().mult_pippenger_prepared(msm.handle, C.byref(out), npoints, _addr(scalars)), "mult_pippenger_prepared")
    return out


def multi_scalar_mult_prepared_batch(msm, scalars, npoints, nbatch):
    out = (BlstP1 * nbatch)()
    _check(lib().mult_pippenger_prepared_batch(msm.handle, out, npoints, nbatch, _addr(scalars)),
           "mult_pippenger_prepared_batch")
    return out


def multi_scalar_mult(points, scalars, npoints):
    """blst-sppark/src/lib.rs:40-62."""
    out = BlstP1()
    _check(lib().mult_pippenger(C.byref(out), _addr(points), npoints, _addr(scalars)), "mult_pippenger")
    return out


def msm_prepared_batch_device(msm, d_out, d_scalars, npoints, nbatch, scalars_mont=True, stream=0):
    """Device-resident form: raw device pointers (ints), enqueued on `stream` (hipStream_t as int)."""
    _check(lib().kzgamd_msm_prepared_batch_device(msm.handle, C.c_void_p(d_out), C.c_void_p(d_scalars), npoints, nbatch,
                                                  1 if scalars_mont else 0, C.c_void_p(stream)),
           "kzgamd_msm_prepared_batch_device")


def device_count():
    return lib().kzgamd_device_count()


def set_device(device):
    """GPU for handles created afterwards by this thread (kzgamd_set_device)."""
    if lib().kzgamd_set_device(device) != 0:
        raise KzgAmdError("kzgamd_set_device(%d) failed" % device)


def get_device():
    return lib().kzgamd_get_device()


def msm_reserve(handle, npoints, nbatch, stream=0):
    _check(lib().kzgamd_msm_reserve(C.c_void_p(handle), npoints, nbatch, C.c_void_p(stream)), "kzgamd_msm_reserve")


# ---------------------------------------------------------------- c-kzg-4844 surface (B3)
_libc = None


def _fopen(path, mode=b"r"):
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
        _libc.fopen.restype = C.c_void_p
        _libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        _libc.fclose.argtypes = [C.c_void_p]
    f = _libc.fopen(os.fsencode(path), mode)
    if not f:
        raise FileNotFoundError(path)
    return f


class KZGSettings:
    """Owns a CKZGSettings loaded through the library's own load_trusted_setup(_file)."""

    def __init__(self):
        self.c = CKZGSettings()
        self.loaded = False

    @classmethod
    def from_file(cls, path, config=None):
        self = cls()
        self._config = config  # keeps the tuning string alive for the duration of the call
        f = _fopen(path)
        try:
            rc = lib().kzgamd_load_trusted_setup_file_ex(C.byref(self.c), f, _cfgp(config)) if config is not None \
                else lib().load_trusted_setup_file(C.byref(self.c), f)
        finally:
            _libc.fclose(f)
        if rc != C_KZG_OK:
            raise KzgAmdError("load_trusted_setup_file: C_KZG_RET %d" % rc)
        self.loaded = True
        return self

    @classmethod
    def from_bytes(cls, g1_monomial, g1_lagrange, g2_monomial, config=None):
        self = cls()
        if config is not None:
            rc = lib().kzgamd_load_trusted_setup_ex(C.byref(self.c), g1_monomial, len(g1_monomial), g1_lagrange, len(g1_lagrange),
                                                    g2_monomial, len(g2_monomial), 0, _cfgp(config))
        else:
            rc = lib().load_trusted_setup(C.byref(self.c), g1_monomial, len(g1_monomial), g1_lagrange, len(g1_lagrange),
                                          g2_monomial, len(g2_monomial), 0)
        if rc != C_KZG_OK:
            raise KzgAmdError("load_trusted_setup: C_KZG_RET %d" % rc)
        self.loaded = True
        return self

    def msm_handle(self):
        return lib().kzgamd_settings_msm_handle(C.byref(self.c))

    def device(self):
        return lib().kzgamd_settings_device(C.byref(self.c))

    def reserve(self, nblobs, stream=0):
        rc = lib().kzgamd_settings_reserve(C.byref(self.c), nblobs, C.c_void_p(stream))
        if rc != C_KZG_OK:
            raise KzgAmdError("kzgamd_settings_reserve: C_KZG_RET %d" % rc)

    def g1_lagrange_brp(self):
        return (BlstP1 * 4096).from_address(self.c.g1_values_lagrange_brp)

    def g1_lagrange_affine(self):
        """the same points as blst_p1_affine (a loaded setup's points have Z = 1: x and y are the affine coordinates)"""
        jac = self.g1_lagrange_brp()
        aff = (BlstP1Affine * 4096)()
        for i in range(4096):
            aff[i].x, aff[i].y = jac[i].x, jac[i].y
        return aff

    def close(self):
        if self.loaded:
            lib().free_trusted_setup(C.byref(self.c))
            self.loaded = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def blob_to_kzg_commitment(blob: bytes, settings: KZGSettings) -> bytes:
    """blst/src/eip_4844.rs:163-175; raises KzgAmdError on C_KZG_BADARGS."""
    if len(blob) != BYTES_PER_BLOB:
        raise KzgAmdError("blob_to_kzg_commitment: C_KZG_RET %d" % C_KZG_BADARGS)
    out = C.create_string_buffer(48)
    rc = lib().blob_to_kzg_commitment(out, blob, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("blob_to_kzg_commitment: C_KZG_RET %d" % rc)
    return out.raw


def blob_to_kzg_commitment_batch(blobs: bytes, n: int, settings: KZGSettings):
    out = C.create_string_buffer(48 * n)
    rc = lib().kzgamd_blob_to_kzg_commitment_batch(out, blobs, n, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_blob_to_kzg_commitment_batch: C_KZG_RET %d" % rc)
    raw = out.raw  # one copy (out.raw copies the whole buffer at every access)
    return [raw[48 * i:48 * i + 48] for i in range(n)]


def blob_to_kzg_commitment_device(d_out, d_status, d_scratch, d_blobs, n, settings, stream=0):
    rc = lib().kzgamd_blob_to_kzg_commitment_device(C.c_void_p(d_out), C.c_void_p(d_status), C.c_void_p(d_scratch),
                                                    C.c_void_p(d_blobs), n, C.byref(settings.c), C.c_void_p(stream))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_blob_to_kzg_commitment_device: C_KZG_RET %d" % rc)


PROOF_SCRATCH_BYTES = 131072 + 64


def compute_blob_kzg_proof_device(d_proofs, d_status, d_scratch, d_blobs, d_commitments, n, settings, stream=0):
    """device pointers (ints); d_scratch = n * PROOF_SCRATCH_BYTES; enqueued on `stream`, not synchronised"""
    rc = lib().kzgamd_compute_blob_kzg_proof_device(C.c_void_p(d_proofs), C.c_void_p(d_status), C.c_void_p(d_scratch),
                                                    C.c_void_p(d_blobs), C.c_void_p(d_commitments), n, C.byref(settings.c),
                                                    C.c_void_p(stream))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_compute_blob_kzg_proof_device: C_KZG_RET %d" % rc)


def msm_set_profile(handle, on=True):
    lib().kzgamd_msm_set_profile(C.c_void_p(handle), 1 if on else 0)


def msm_get_profile(handle):
    """(avg k_accum ms, avg whole-enqueue ms, enqueues averaged) or None"""
    a, t = C.c_float(), C.c_float()
    cnt = lib().kzgamd_msm_get_profile(C.c_void_p(handle), C.byref(a), C.byref(t))
    if cnt <= 0:
        return None
    return a.value, t.value, cnt


class DeviceMsm(PreparedMsm):
    """Handle over device-resident bases (kzgamd_msm_create_device)."""

    def __init__(self, d_points, npoints, prepare, config=None):
        self.npoints = npoints
        self.handle = lib().kzgamd_msm_create_device_ex(C.c_void_p(d_points), npoints, 1 if prepare else 0, _cfgp(config))
        if not self.handle:
            raise KzgAmdError("kzgamd_msm_create_device failed")


def generate_points(d_out, npoints, seed, stream=0):
    _check(lib().kzgamd_generate_points(C.c_void_p(d_out), npoints, seed, C.c_void_p(stream)), "kzgamd_generate_points")


# ---------------------------------------------------------------- NTT plug-in (B2)
def g1_sum(points):
    """Sum of Jacobian blst_p1 values given as 144-byte strings (host arithmetic; the combine step of msm_sharded)."""
    n = len(points)
    buf = (BlstP1 * max(n, 1))()
    for i, pt in enumerate(points):
        C.memmove(C.byref(buf[i]), bytes(pt), 144)
    out = BlstP1()
    lib().kzgamd_g1_sum(C.byref(out), buf, n)
    return bytes(out)


class FFTSettings:
    """Mirror of FsFFTSettings (blst/src/types/fft_settings.rs:14-58) + FFTFr / DASExtension
    (blst/src/fft_fr.rs:156-165, blst/src/data_availability_sampling.rs:78-100).
    Errors are raised with the reference's messages."""

    def __init__(self, scale, config=None):
        if scale >= 32:
            raise KzgAmdError("Scale is expected to be within root of unity matrix row size")
        self.scale = scale
        self.max_width = 1 << scale
        self.handle = lib().kzgamd_ntt_new_ex(scale, _cfgp(config)) if config is not None else lib().kzgamd_ntt_new(scale)
        if not self.handle:
            raise KzgAmdError("kzgamd_ntt_new failed (no GPU?)")

    def fft_fr(self, data, n, inverse=False):
        """data: blst_fr[n] (ctypes array / buffer). Returns a new (BlstFr * n)."""
        out = (BlstFr * max(n, 1))()
        rc = lib().ntt_fr(self.handle, out, _addr(data), n, 1 if inverse else 0)
        if rc == 1:
            raise KzgAmdError("Supplied list is longer than the available max width")
        if rc == 2:
            raise KzgAmdError("A list with power-of-two length expected")
        if rc != 0:
            raise KzgAmdError("ntt_fr: device error %d" % rc)
        return out

    def fft_g1(self, data, n, inverse=False, nbatch=1):
        """FFTG1::fft_g1 (blst/src/fft_g1.rs:54-83). data: blst_p1[n * nbatch]. Returns a new (BlstP1 * (n * nbatch))."""
        out = (BlstP1 * max(n * nbatch, 1))()
        if nbatch == 1:
            rc = lib().fft_g1(self.handle, out, _addr(data), n, 1 if inverse else 0)
        else:
            rc = lib().kzgamd_fft_g1_batch(self.handle, out, _addr(data), n, nbatch, 1 if inverse else 0)
        if rc == 1:
            raise KzgAmdError("Supplied list is longer than the available max width")
        if rc == 2:
            raise KzgAmdError("A list with power-of-two length expected")
        if rc != 0:
            raise KzgAmdError("fft_g1: device error %d" % rc)
        return out

    def das_fft_extension(self, evens, n):
        out = (BlstFr * max(n, 1))()
        rc = lib().das_fft_extension(self.handle, out, _addr(evens), n)
        if rc == 1:
            raise KzgAmdError("A non-zero list ab expected")
        if rc == 2:
            raise KzgAmdError("A list with power-of-two length expected")
        if rc == 3:
            raise KzgAmdError("Supplied list is longer than the available max width")
        if rc != 0:
            raise KzgAmdError("das_fft_extension: device error %d" % rc)
        return out

    def fft_fr_device(self, d_out, d_in, n, nbatch=1, inverse=False, stream=0):
        rc = lib().kzgamd_ntt_fr_device(self.handle, C.c_void_p(d_out), C.c_void_p(d_in), n, nbatch, 1 if inverse else 0,
                                        C.c_void_p(stream))
        if rc != 0:
            raise KzgAmdError("kzgamd_ntt_fr_device: %d" % rc)

    def das_fft_extension_device(self, d_odds, d_evens, d_scratch, half_n, nbatch=1, stream=0):
        rc = lib().kzgamd_das_fft_extension_device(self.handle, C.c_void_p(d_odds), C.c_void_p(d_evens), C.c_void_p(d_scratch),
                                                   half_n, nbatch, C.c_void_p(stream))
        if rc != 0:
            raise KzgAmdError("kzgamd_das_fft_extension_device: %d" % rc)

    def roots(self):
        W = self.max_width
        r, rr, br = (BlstFr * (W + 1))(), (BlstFr * (W + 1))(), (BlstFr * W)()
        lib().kzgamd_ntt_roots(self.handle, r, rr, br)
        return r, rr, br

    def close(self):
        if self.handle:
            lib().kzgamd_ntt_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FK20_ERRORS = {
    1: "n2 must be less than or equal to kzg settings max width",
    2: "n2 must be a power of two",
    3: "n2 must be greater than or equal to 2",
    4: "chunk_len must be greater or equal to n2 / 2",
    5: "chunk_len must be a power of two",
    6: "the setup has fewer than n2 / 2 - chunk_len G1 points",
}


class FK20Settings:
    """FK20SingleSettings (chunk_len = 1) / FK20MultiSettings of the reference over an FFTSettings handle
    (blst/src/types/fk20_single_settings.rs, fk20_multi_settings.rs); errors carry the reference's messages.  Keeps the
    FFTSettings object alive; close() (or leaving the `with` block) frees the GPU state."""

    def __init__(self, fft_settings, g1_monomial, num_g1, n2, chunk_len=1, config=None):
        self.fs = fft_settings
        self.handle = None
        err = C.c_int(0)
        self.handle = lib().kzgamd_fk20_new(fft_settings.handle, _addr(g1_monomial), num_g1, n2, chunk_len, _cfgp(config), C.byref(err))
        self.err = err.value
        if not self.handle:
            raise KzgAmdError(FK20_ERRORS.get(err.value, "kzgamd_fk20_new failed: %d (no GPU, bad configuration, or fk20_table=1 without room)" % err.value))
        self.n2, self.chunk_len = n2, chunk_len

    @classmethod
    def new(cls, fft_settings, g1_monomial, num_g1, n2, chunk_len=1, config=None):
        return cls(fft_settings, g1_monomial, num_g1, n2, chunk_len, config)

    def data_availability(self, polys, npoly=1, optimized=False):
        """polys: blst_fr[npoly * n2/2] (Montgomery).  Returns a new (BlstP1 * (npoly * n2/chunk_len)), Jacobian:
        bit-reversed per polynomial (data_availability) or in natural order (optimized=True)."""
        if not self.handle:
            raise KzgAmdError("FK20Settings is closed")
        n = self.n2 // 2
        out = (BlstP1 * max(1, npoly * (self.n2 // self.chunk_len)))()
        rc = lib().kzgamd_fk20_da(self.handle, out, _addr(polys), n, npoly, 1 if optimized else 0)
        if rc != 0:
            raise KzgAmdError("kzgamd_fk20_da: %d" % rc)
        return out

    def info(self):
        """(n2, chunk_len, form): form 1 = a scalar multiplication per product, 2 = wide fixed-base table"""
        a, b, f = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        if lib().kzgamd_fk20_info(self.handle, C.byref(a), C.byref(b), C.byref(f)) != 0:
            raise KzgAmdError("kzgamd_fk20_info failed")
        return a.value, b.value, f.value

    def close(self):
        if self.handle:
            lib().kzgamd_fk20_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KZG_ERRORS = {
    1: "Polynomial is longer than secret g1",
    2: "Polynomial must not be empty",
    3: "n must be a power of two",
    4: "Supplied list is longer than the available max width",
    5: "x must not be zero: the interpolation on the coset divides by it",
    6: "the setup has too few G2 points",
    7: "a commitment or proof is not on the curve or not in G1",
}


def _one_fr(r):
    """NULL, or the address of one BlstFr (a BlstFr or any buffer of 32 bytes)"""
    if r is None:
        return None
    return C.cast(C.pointer(r), C.c_void_p) if isinstance(r, C.Structure) else _addr(r)


def batch_challenge(commitments, proofs, xs, ys, n=1, count=1):
    """The weight base r of PolyKZGSettings.check_batch(r=None): hash_to_bls_field(SHA-256("KZGAMD_CHKBATCH1" | u64_be(n) |
    u64_be(count) | commitments | proofs | xs | ys)) over the buffers' bytes as passed.  Host only.  Returns a BlstFr."""
    out = BlstFr()
    rc = lib().kzgamd_kzg_batch_challenge(C.byref(out), _addr(commitments) if count else None, _addr(proofs) if count else None,
                                          _addr(xs) if count else None, _addr(ys) if count * n else None, n, count)
    if rc != 0:
        raise KzgAmdError("kzgamd_kzg_batch_challenge: %d" % rc)
    return out


class PolyKZGSettings:
    """The proving and checking calls of the reference's KZGSettings (blst/src/types/kzg_settings.rs:138-277) over an
    FFTSettings handle and a monomial setup, batched; errors carry the reference's messages.  Keeps the FFTSettings
    object alive; close() (or leaving the `with` block) frees the GPU state."""

    def __init__(self, fft_settings, g1_monomial, num_g1, g2_monomial=None, num_g2=0, config=None):
        self.fs = fft_settings
        self.handle = None
        err = C.c_int(0)
        g2 = _addr(g2_monomial) if g2_monomial is not None and num_g2 else None
        self.handle = lib().kzgamd_kzg_new(fft_settings.handle, _addr(g1_monomial) if num_g1 else None, num_g1, g2,
                                           num_g2 if g2 else 0, _cfgp(config), C.byref(err))
        self.err = err.value
        if not self.handle:
            raise KzgAmdError("the setup has no G1 points" if err.value == 1 else
                              "kzgamd_kzg_new failed: %d (no GPU, NULL argument or bad configuration)" % err.value)

    def _live(self):
        if not self.handle:
            raise KzgAmdError("PolyKZGSettings is closed")

    @staticmethod
    def _raise(what, rc):
        raise KzgAmdError(KZG_ERRORS.get(rc, "%s: %d" % (what, rc)))

    def commit(self, polys, length, npoly=1):
        """commit_to_poly for npoly polynomials of `length` Montgomery coefficients each.  Returns (BlstP1 * npoly)."""
        self._live()
        out = (BlstP1 * max(1, npoly))()
        rc = lib().kzgamd_kzg_commit(self.handle, out, _addr(polys) if npoly * length else None, length, npoly)
        if rc != 0:
            self._raise("kzgamd_kzg_commit", rc)
        return out

    def open(self, polys, length, npoly, xs, nx, n=1, want_ys=True):
        """compute_proof_single (n = 1) / compute_proof_multi for every (polynomial, x) pair.  Returns
        (proofs: BlstP1 * (npoly * nx), ys: BlstFr * (npoly * nx * n) or None); ys[(b * nx + k) * n + i] = p_b(x_k w^i)."""
        self._live()
        pairs = npoly * nx
        proofs = (BlstP1 * max(1, pairs))()
        ys = (BlstFr * max(1, pairs * n))() if want_ys else None
        rc = lib().kzgamd_kzg_open(self.handle, proofs, ys, _addr(polys) if npoly * length else None, length, npoly,
                                   _addr(xs) if nx else None, nx, n)
        if rc != 0:
            self._raise("kzgamd_kzg_open", rc)
        return proofs, ys

    def check(self, commitments, proofs, xs, ys, n=1, count=1):
        """check_proof_single (n = 1) / check_proof_multi for `count` tuples.  Returns a list of count booleans."""
        self._live()
        ok = (C.c_bool * max(1, count))()
        rc = lib().kzgamd_kzg_check(self.handle, ok, _addr(commitments), _addr(proofs), _addr(xs), _addr(ys), n, count)
        if rc != 0:
            self._raise("kzgamd_kzg_check", rc)
        return [bool(ok[i]) for i in range(count)]

    def check_batch(self, commitments, proofs, xs, ys, n=1, count=1, r=None, each=False):
        """All `count` tuples under one pairing, weighted by the powers of r (None: batch_challenge of the inputs; a
        caller's own r must be fixed after the inputs are).  Returns the verdict, or (verdict, list of count booleans)
        with each=True — all true when the batch passes, check()'s when it fails."""
        self._live()
        ok = C.c_bool(False)
        per = (C.c_bool * max(1, count))() if each else None
        rc = lib().kzgamd_kzg_check_batch(self.handle, C.byref(ok), per, _addr(commitments), _addr(proofs), _addr(xs), _addr(ys),
                                          n, count, _one_fr(r))
        if rc != 0:
            self._raise("kzgamd_kzg_check_batch", rc)
        return (ok.value, [bool(per[i]) for i in range(count)]) if each else ok.value

    def check_batch_g1(self, commitments, proofs, xs, ys, n=1, count=1, r=None):
        """The two G1 sides of check_batch, no pairing: (BlstP1 * 2) = L, P with e(L, G2) == e(P, [s^n]G2) the verdict."""
        self._live()
        out = (BlstP1 * 2)()
        rc = lib().kzgamd_kzg_check_batch_g1(self.handle, out, _addr(commitments), _addr(proofs), _addr(xs), _addr(ys), n, count,
                                             _one_fr(r))
        if rc != 0:
            self._raise("kzgamd_kzg_check_batch_g1", rc)
        return out

    def info(self):
        """(num_g1, num_g2, chunk, lane_form_min): the setup sizes, the chunk length of the scan form of the quotient
        kernels and the number of lanes (pairs x n) from which the lane form is taken"""
        self._live()
        v = [C.c_size_t(0) for _ in range(4)]
        if lib().kzgamd_kzg_info(self.handle, *[C.byref(x) for x in v]) != 0:
            raise KzgAmdError("kzgamd_kzg_info failed")
        return tuple(x.value for x in v)

    def close(self):
        if self.handle:
            lib().kzgamd_kzg_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


POLY_ERRORS = {
    "inverse": {1: "Can't produce a zero-length result", 2: "Can't inverse a zero-length poly",
                3: "First coefficient of polynomial mustn't be zero"},
    "div": {1: "Can't divide by zero", 2: "Highest coefficient must be non-zero"},
    # blst/src/zero_poly.rs, blst/src/recovery.rs; where the reference panics the message says what it trips over
    "zero_partial": {1: "idx array must not be empty", 2: "index out of bounds: idx * stride exceeds max_width"},
    "reduce_partials": {1: "Expected domain size to be a power of 2", 2: "partials must not be empty",
                        3: "Out degree is longer than possible polynomial size in domain",
                        4: "Domain size greater than fft_settings.max_width", 5: "attempt to subtract with overflow: empty partial"},
    "zero_poly": {1: "Missing idxs greater than domain size", 2: "Domain size greater than fft_settings.max_width",
                  3: "Domain size must be a power of 2", 5: "index out of bounds: missing idx exceeds domain size"},
    "recover": {1: "Samples must have a length that is a power of two", 2: "Impossible to recover, too many shards are missing",
                3: "Supplied list is longer than the available max width"},
}


class PolySettings:
    """The reference's Poly<Fr> and FFTSettingsPoly (blst/src/types/poly.rs) over an FFTSettings handle, batched: every
    call takes npoly polynomials of one shape, contiguous, as Montgomery blst_fr.  Errors carry the reference's messages
    and the code (`.code`).  Keeps the FFTSettings object alive; close() (or leaving the `with` block) frees the GPU state."""

    def __init__(self, fs, config=None):
        self.fs = fs
        self.handle = None
        err = C.c_int(0)
        self.handle = lib().kzgamd_poly_new(fs.handle, _cfgp(config), C.byref(err))
        self.err = err.value
        if not self.handle:
            raise self._error("kzgamd_poly_new", err.value, "kzgamd_poly_new failed: %d (no GPU, NULL argument or bad configuration)" % err.value)

    @staticmethod
    def _error(what, rc, msg=None):
        if msg is None and rc == 4:
            msg = "Supplied list is longer than the available max width"
        e = KzgAmdError(msg or "%s: %d" % (what, rc))
        e.code = rc
        return e

    def _live(self):
        if not self.handle:
            raise KzgAmdError("PolySettings is closed")

    def eval(self, polys, length, npoly, xs, nx):
        """Poly::eval of every polynomial at every x.  Returns (BlstFr * (npoly * nx)): ys[b * nx + k] = p_b(x_k)."""
        self._live()
        ys = (BlstFr * max(1, npoly * nx))()
        rc = lib().kzgamd_poly_eval(self.handle, ys, _addr(polys) if npoly * length else None, length, npoly,
                                    _addr(xs) if nx else None, nx)
        if rc != 0:
            raise self._error("kzgamd_poly_eval", rc)
        return ys

    def scale(self, polys, length, npoly=1, inverse=False):
        """Poly::scale (coefficient i times 5^-(i+1)) or, inverse=True, Poly::unscale.  Returns (BlstFr * (npoly * length))."""
        self._live()
        out = (BlstFr * max(1, npoly * length))()
        rc = lib().kzgamd_poly_scale(self.handle, out, _addr(polys) if npoly * length else None, length, npoly, 1 if inverse else 0)
        if rc != 0:
            raise self._error("kzgamd_poly_scale", rc)
        return out

    def mul(self, a, la, b, lb, out_len, npoly=1, form=0):
        """The first out_len coefficients of a_b * b_b (Poly::mul; form 1: mul_direct, 2: mul_fft).  Returns
        (BlstFr * (npoly * out_len))."""
        self._live()
        out = (BlstFr * max(1, npoly * out_len))()
        rc = lib().kzgamd_poly_mul(self.handle, out, _addr(a) if npoly * la else None, la, _addr(b) if npoly * lb else None, lb,
                                   out_len, npoly, form)
        if rc != 0:
            raise self._error("kzgamd_poly_mul", rc)
        return out

    def inverse(self, b, lb, out_len, npoly=1):
        """Poly::inverse: the first out_len coefficients of 1 / b_b.  Returns (BlstFr * (npoly * out_len))."""
        self._live()
        out = (BlstFr * max(1, npoly * out_len))()
        rc = lib().kzgamd_poly_inverse(self.handle, out, _addr(b) if npoly * lb else None, lb, out_len, npoly)
        if rc != 0:
            raise self._error("kzgamd_poly_inverse", rc, POLY_ERRORS["inverse"].get(rc))
        return out

    def div(self, a, la, b, lb, npoly=1):
        """Poly::div: the quotients of a_b by b_b.  Returns (BlstFr * (npoly * (la - lb + 1))), of length 0 when la < lb."""
        self._live()
        qlen = la - lb + 1 if la >= lb else 0
        out = (BlstFr * (npoly * qlen))()
        rc = lib().kzgamd_poly_div(self.handle, out, _addr(a) if npoly * la else None, la, _addr(b) if npoly * lb else None, lb, npoly)
        if rc != 0:
            raise self._error("kzgamd_poly_div", rc, POLY_ERRORS["div"].get(rc))
        return out

    def info(self):
        """(max_width, eval_chunk, mul_direct_max, inv_direct_max): see kzgamd_poly_info"""
        self._live()
        v = [C.c_size_t(0) for _ in range(4)]
        if lib().kzgamd_poly_info(self.handle, *[C.byref(x) for x in v]) != 0:
            raise KzgAmdError("kzgamd_poly_info failed")
        return tuple(x.value for x in v)

    def zero_partial(self, idxs, stride=1):
        """do_zero_poly_mul_partial for any number of indices: the len(idxs) + 1 coefficients of
        prod (X - roots[idx * stride]).  Returns (BlstFr * (len(idxs) + 1))."""
        self._live()
        n = len(idxs)
        arr = (C.c_uint64 * max(1, n))(*idxs)
        out = (BlstFr * (n + 1))()
        rc = lib().kzgamd_poly_zero_partial(self.handle, out, arr, n, stride)
        if rc != 0:
            raise self._error("kzgamd_poly_zero_partial", rc, POLY_ERRORS["zero_partial"].get(rc))
        return out

    def reduce_partials(self, domain_size, partials, lens):
        """reduce_partials: the product of len(lens) polynomials stored back to back in `partials` (blst_fr, Montgomery).
        Returns (BlstFr * (sum(lens) - len(lens) + 1))."""
        self._live()
        m = len(lens)
        larr = (C.c_size_t * max(1, m))(*lens)
        out = (BlstFr * max(1, sum(lens) - m + 1))()
        rc = lib().kzgamd_poly_reduce_partials(self.handle, out, domain_size, _addr(partials) if sum(lens) else None, larr, m)
        if rc != 0:
            raise self._error("kzgamd_poly_reduce_partials", rc, POLY_ERRORS["reduce_partials"].get(rc))
        return out

    def zero_poly(self, domain_size, missing_lists, form=0, want_eval=True, want_poly=True):
        """zero_poly_via_multiplication for every index list of missing_lists in one call.  Returns (zero_eval, zero_poly),
        each (BlstFr * (len(missing_lists) * domain_size)) or None when not wanted.  An empty list gives the empty
        product (the reference returns two empty vectors there)."""
        self._live()
        nprob = len(missing_lists)
        flat = [i for lst in missing_lists for i in lst]
        offs = [0]
        for lst in missing_lists:
            offs.append(offs[-1] + len(lst))
        marr = (C.c_uint64 * max(1, len(flat)))(*flat)
        oarr = (C.c_size_t * (nprob + 1))(*offs)
        ze = (BlstFr * max(1, nprob * domain_size))() if want_eval else None
        zp = (BlstFr * max(1, nprob * domain_size))() if want_poly else None
        rc = lib().kzgamd_poly_zero_poly(self.handle, ze, zp, domain_size, marr, oarr, nprob, form)
        if rc != 0:
            raise self._error("kzgamd_poly_zero_poly", rc, POLY_ERRORS["zero_poly"].get(rc))
        return ze, zp

    def recover(self, samples, present, n, nprob=1, coeffs=False):
        """recover_poly_from_samples (coeffs=True: recover_poly_coeffs_from_samples) for nprob vectors of n samples
        (blst_fr, Montgomery); present: nprob * n bytes, 0 marks a missing sample, whose value is never used.
        Returns (BlstFr * (nprob * n))."""
        self._live()
        mask = (C.c_uint8 * max(1, nprob * n)).from_buffer_copy(bytes(present) if nprob * n else b"\0")
        out = (BlstFr * max(1, nprob * n))()
        rc = lib().kzgamd_poly_recover(self.handle, out, _addr(samples) if nprob * n else None, mask, n, nprob, 1 if coeffs else 0)
        if rc != 0:
            raise self._error("kzgamd_poly_recover", rc, POLY_ERRORS["recover"].get(rc))
        return out

    def zero_info(self):
        """(leaf_roots, direct_max): see kzgamd_poly_zero_info"""
        self._live()
        v = [C.c_size_t(0) for _ in range(2)]
        if lib().kzgamd_poly_zero_info(self.handle, *[C.byref(x) for x in v]) != 0:
            raise KzgAmdError("kzgamd_poly_zero_info failed")
        return tuple(x.value for x in v)

    @staticmethod
    def zero_plan(count):
        """the levels the tree form runs for `count` roots: [(polynomials entering, coefficients each, transform length)].  No GPU."""
        lv = (C.c_size_t * 96)()
        k = lib().kzgamd_poly_zero_plan(count, lv)
        return [(lv[3 * i], lv[3 * i + 1], lv[3 * i + 2]) for i in range(k)]

    @staticmethod
    def transform_len(op, la, lb, out_len):
        """the longest transform a call of this shape enqueues (0: none); op "mul" (form 2), "inverse" or "div".  No GPU."""
        return lib().kzgamd_poly_transform_len({"mul": 0, "inverse": 1, "div": 2}[op], la, lb, out_len)

    def close(self):
        if self.handle:
            lib().kzgamd_poly_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compute_kzg_proof(blob: bytes, z: bytes, settings: KZGSettings):
    """blst/src/eip_4844.rs:476-496 -> (proof48, y32)"""
    if len(blob) != BYTES_PER_BLOB or len(z) != 32:
        raise KzgAmdError("compute_kzg_proof: C_KZG_RET %d" % C_KZG_BADARGS)
    proof, y = C.create_string_buffer(48), C.create_string_buffer(32)
    rc = lib().compute_kzg_proof(proof, y, blob, z, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("compute_kzg_proof: C_KZG_RET %d" % rc)
    return proof.raw, y.raw


def compute_blob_kzg_proof(blob: bytes, commitment: bytes, settings: KZGSettings) -> bytes:
    """blst/src/eip_4844.rs:274-291"""
    if len(blob) != BYTES_PER_BLOB or len(commitment) != 48:
        raise KzgAmdError("compute_blob_kzg_proof: C_KZG_RET %d" % C_KZG_BADARGS)
    proof = C.create_string_buffer(48)
    rc = lib().compute_blob_kzg_proof(proof, blob, commitment, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("compute_blob_kzg_proof: C_KZG_RET %d" % rc)
    return proof.raw


def compute_blob_kzg_proof_batch(blobs: bytes, commitments: bytes, n: int, settings: KZGSettings):
    """New batched API (BASELINE.json configs[4]); equals n compute_blob_kzg_proof calls."""
    out = C.create_string_buffer(48 * n)
    rc = lib().kzgamd_compute_blob_kzg_proof_batch(out, blobs, commitments, n, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_compute_blob_kzg_proof_batch: C_KZG_RET %d" % rc)
    raw = out.raw  # one copy (out.raw copies the whole buffer at every access)
    return [raw[48 * i:48 * i + 48] for i in range(n)]


def compute_challenges_and_evaluate_batch(blobs: bytes, commitments: bytes, n: int, settings: KZGSettings):
    """compute_challenges_and_evaluate_polynomial (kzg/src/eip_4844.rs:690-719): per blob the Fiat-Shamir challenge z
    and y = p(z), 32-byte big-endian each — the field work of verify_blob_kzg_proof_batch."""
    zs, ys = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
    rc = lib().kzgamd_compute_challenges_and_evaluate_batch(zs, ys, blobs, commitments, n, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_compute_challenges_and_evaluate_batch: C_KZG_RET %d" % rc)
    zr, yr = zs.raw, ys.raw
    return ([zr[32 * i:32 * i + 32] for i in range(n)], [yr[32 * i:32 * i + 32] for i in range(n)])


def verify_kzg_proof_batch_g1(commitments: bytes, zs: bytes, ys: bytes, proofs: bytes, n: int, settings: KZGSettings):
    """verify_kzg_proof_batch (kzg/src/eip_4844.rs:380-435) up to the pairing -> (proof_lincomb, rhs) as BlstP1."""
    a, b = BlstP1(), BlstP1()
    rc = lib().kzgamd_verify_kzg_proof_batch_g1(C.byref(a), C.byref(b), commitments, zs, ys, proofs, n, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_verify_kzg_proof_batch_g1: C_KZG_RET %d" % rc)
    return a, b


def verify_blob_kzg_proof_batch_g1(blobs: bytes, commitments: bytes, proofs: bytes, n: int, settings: KZGSettings):
    """verify_blob_kzg_proof_batch (kzg/src/eip_4844.rs:736-832) up to the pairing -> (proof_lincomb, rhs)."""
    a, b = BlstP1(), BlstP1()
    rc = lib().kzgamd_verify_blob_kzg_proof_batch_g1(C.byref(a), C.byref(b), blobs, commitments, proofs, n, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_verify_blob_kzg_proof_batch_g1: C_KZG_RET %d" % rc)
    return a, b


def _verdict(rc, ok, what):
    if rc != C_KZG_OK:
        raise KzgAmdError("%s: C_KZG_RET %d" % (what, rc))
    return bool(ok.value)


def verify_kzg_proof(commitment: bytes, z: bytes, y: bytes, proof: bytes, settings: KZGSettings) -> bool:
    """blst/src/eip_4844.rs:383-405"""
    if len(commitment) != 48 or len(z) != 32 or len(y) != 32 or len(proof) != 48:
        raise KzgAmdError("verify_kzg_proof: C_KZG_RET %d" % C_KZG_BADARGS)
    ok = C.c_bool(False)
    return _verdict(lib().verify_kzg_proof(C.byref(ok), commitment, z, y, proof, C.byref(settings.c)), ok, "verify_kzg_proof")


def verify_blob_kzg_proof(blob: bytes, commitment: bytes, proof: bytes, settings: KZGSettings) -> bool:
    """blst/src/eip_4844.rs:410-430"""
    if len(blob) != BYTES_PER_BLOB or len(commitment) != 48 or len(proof) != 48:
        raise KzgAmdError("verify_blob_kzg_proof: C_KZG_RET %d" % C_KZG_BADARGS)
    ok = C.c_bool(False)
    return _verdict(lib().verify_blob_kzg_proof(C.byref(ok), blob, commitment, proof, C.byref(settings.c)), ok,
                    "verify_blob_kzg_proof")


def verify_blob_kzg_proof_batch(blobs, commitments, proofs, settings: KZGSettings) -> bool:
    """blst/src/eip_4844.rs:435-471; lists of bytes.  Length mismatches are the reference's 'Invalid amount of arguments'."""
    n = len(blobs)
    if len(commitments) != n or len(proofs) != n or any(len(b) != BYTES_PER_BLOB for b in blobs) or \
            any(len(c) != 48 for c in commitments) or any(len(p) != 48 for p in proofs):
        raise KzgAmdError("verify_blob_kzg_proof_batch: C_KZG_RET %d" % C_KZG_BADARGS)
    ok = C.c_bool(False)
    return _verdict(lib().verify_blob_kzg_proof_batch(C.byref(ok), b"".join(blobs), b"".join(commitments), b"".join(proofs), n,
                                                      C.byref(settings.c)), ok, "verify_blob_kzg_proof_batch")


def pairings_verify(a1, a2, b1, b2) -> bool:
    """blst/src/kzg_proofs.rs:73-100 on BlstP1 / BlstP2 values (host arithmetic, no GPU)."""
    rc = lib().kzgamd_pairings_verify(C.byref(a1), C.byref(a2), C.byref(b1), C.byref(b2))
    if rc < 0:
        raise KzgAmdError("kzgamd_pairings_verify")
    return rc == 1


def pairings_verify_batch(a1, a2, b1, b2):
    """[e(a1[i], a2) == e(b1[i], b2)] for sequences (or ctypes arrays) of BlstP1 against two shared BlstP2 values, on the
    GPU, one wave per check: kzgamd_pairings_verify's verdicts item by item."""
    n = len(a1)
    if len(b1) != n:
        raise KzgAmdError("kzgamd_pairings_verify_batch: %d against %d G1 points" % (n, len(b1)))
    if n == 0:
        return []
    aa = a1 if isinstance(a1, C.Array) else (BlstP1 * n)(*a1)
    bb = b1 if isinstance(b1, C.Array) else (BlstP1 * n)(*b1)
    ok = (C.c_bool * n)()
    rc = lib().kzgamd_pairings_verify_batch(ok, aa, C.byref(a2), bb, C.byref(b2), n)
    if rc != 0:
        raise KzgAmdError("kzgamd_pairings_verify_batch: %d" % rc)
    return [bool(v) for v in ok]


def pairing_info() -> int:
    """the checks one launch of pairings_verify_batch takes (larger batches run in slices)"""
    out = C.c_size_t(0)
    lib().kzgamd_pairing_info(C.byref(out))
    return out.value


def p2_uncompress(b: bytes) -> BlstP2:
    out = BlstP2()
    if len(b) != 96 or lib().kzgamd_p2_uncompress(C.byref(out), b) != 0:
        raise KzgAmdError("kzgamd_p2_uncompress: invalid G2 encoding")
    return out


def p2_compress(p) -> bytes:
    out = C.create_string_buffer(96)
    lib().kzgamd_p2_compress(out, C.byref(p))
    return out.raw


def p2_generator() -> BlstP2:
    out = BlstP2()
    lib().kzgamd_p2_generator(C.byref(out))
    return out


def p2_mult(p, fr) -> BlstP2:
    out = BlstP2()
    lib().kzgamd_p2_mult(C.byref(out), C.byref(p), C.byref(fr))
    return out


def p2_add(a, b) -> BlstP2:
    out = BlstP2()
    lib().kzgamd_p2_add(C.byref(out), C.byref(a), C.byref(b))
    return out


def _group_mul_check(rc, what):
    if rc == 1:
        raise KzgAmdError("%s: the Lagrange form needs an FFTSettings and a power-of-two number of G1 points" % what)
    if rc == 2:
        raise KzgAmdError("Supplied list is longer than the available max width")
    if rc == 3:
        raise KzgAmdError("%s: the base is not in the G1 subgroup" % what)
    if rc != 0:
        raise KzgAmdError("%s: %d" % (what, rc))


def g1_mul_batch(scalars, n, base=None, config=None):
    """out[i] = scalars[i] * base on the GPU (base None: the generator).  scalars: blst_fr[n] in Montgomery form (ctypes
    array / buffer), base: a BlstP1 of the subgroup.  Returns a new (BlstP1 * n)."""
    out = (BlstP1 * max(n, 1))()
    rc = lib().kzgamd_g1_mul_batch(out, C.byref(base) if base is not None else None, _addr(scalars) if n else None, n, _cfgp(config))
    _group_mul_check(rc, "kzgamd_g1_mul_batch")
    return out


def g2_mul_batch(scalars, n, base=None, config=None):
    """the same in G2: base a BlstP2 of the subgroup (not tested), returns a new (BlstP2 * n)."""
    out = (BlstP2 * max(n, 1))()
    rc = lib().kzgamd_g2_mul_batch(out, C.byref(base) if base is not None else None, _addr(scalars) if n else None, n, _cfgp(config))
    _group_mul_check(rc, "kzgamd_g2_mul_batch")
    return out


def generate_trusted_setup(num_g1, secret, num_g2=None, fft_settings=None, want_lagrange=True, config=None):
    """generate_trusted_setup of the reference (blst/src/utils.rs:16-37) on the GPU: ([s^i]G1 as BlstP1 * num_g1, their
    Lagrange form (or None), [s^j]G2 as BlstP2 * num_g2) for s = the 32 bytes `secret` as a big-endian integer mod r.
    num_g2 None: num_g1, as the reference.  The Lagrange form takes an FFTSettings of at least num_g1 points."""
    if len(secret) != 32:
        raise KzgAmdError("generate_trusted_setup: the secret is 32 bytes")
    num_g2 = num_g1 if num_g2 is None else num_g2
    mono = (BlstP1 * max(num_g1, 1))()
    lag = (BlstP1 * max(num_g1, 1))() if want_lagrange else None
    g2 = (BlstP2 * max(num_g2, 1))()
    rc = lib().kzgamd_generate_trusted_setup(fft_settings.handle if fft_settings is not None else None, mono, lag, g2, num_g1, num_g2,
                                             bytes(secret), _cfgp(config))
    _group_mul_check(rc, "kzgamd_generate_trusted_setup")
    return mono, lag, g2


def group_mul_info():
    """{"slice_points", "g1_window_bits", "g2_window_bits"} of g1_mul_batch / g2_mul_batch / generate_trusted_setup"""
    s, a, b = C.c_size_t(0), C.c_int(0), C.c_int(0)
    lib().kzgamd_group_mul_info(C.byref(s), C.byref(a), C.byref(b))
    return {"slice_points": s.value, "g1_window_bits": a.value, "g2_window_bits": b.value}


def _codec_check(rc, what):
    if rc not in (0, 1):
        raise KzgAmdError("%s: %d" % (what, rc))
    return rc


def g1_compress_batch(points, n, config=None) -> bytes:
    """the n Jacobian BlstP1 of `points` (ctypes array / buffer) as 48 bytes each, compressed on the GPU"""
    out = C.create_string_buffer(48 * max(n, 1))
    _codec_check(lib().kzgamd_g1_compress_batch(out, _addr(points) if n else None, n, _cfgp(config)), "kzgamd_g1_compress_batch")
    return out.raw[:48 * n]


def g1_to_affine_batch(points, n, config=None):
    """the same points as a new (BlstP1Affine * n); the identity is (0, 0)"""
    out = (BlstP1Affine * max(n, 1))()
    _codec_check(lib().kzgamd_g1_to_affine_batch(out, _addr(points) if n else None, n, _cfgp(config)), "kzgamd_g1_to_affine_batch")
    return out


def g1_uncompress_batch(data: bytes, check_subgroup=True, config=None):
    """len(data) / 48 compressed G1 points parsed on the GPU: (BlstP1 * n, status bytes, rc).  status[i]: 0 ok, 1 not a
    valid encoding, 2 (check_subgroup) outside the subgroup; refused entries are all-zero; rc is 1 when any was refused."""
    if len(data) % 48:
        raise KzgAmdError("g1_uncompress_batch: the input is not a whole number of 48-byte points")
    n = len(data) // 48
    out = (BlstP1 * max(n, 1))()
    status = C.create_string_buffer(max(n, 1))
    rc = _codec_check(lib().kzgamd_g1_uncompress_batch(out, status, bytes(data), n, 1 if check_subgroup else 0, _cfgp(config)),
                      "kzgamd_g1_uncompress_batch")
    return out, status.raw[:n], rc


def g2_compress_batch(points, n, config=None) -> bytes:
    """the n Jacobian BlstP2 of `points` as 96 bytes each, compressed on the GPU"""
    out = C.create_string_buffer(96 * max(n, 1))
    _codec_check(lib().kzgamd_g2_compress_batch(out, _addr(points) if n else None, n, _cfgp(config)), "kzgamd_g2_compress_batch")
    return out.raw[:96 * n]


def g2_uncompress_batch(data: bytes, check_subgroup=True, config=None):
    """as g1_uncompress_batch for 96-byte G2 points: (BlstP2 * n, status bytes, rc)"""
    if len(data) % 96:
        raise KzgAmdError("g2_uncompress_batch: the input is not a whole number of 96-byte points")
    n = len(data) // 96
    out = (BlstP2 * max(n, 1))()
    status = C.create_string_buffer(max(n, 1))
    rc = _codec_check(lib().kzgamd_g2_uncompress_batch(out, status, bytes(data), n, 1 if check_subgroup else 0, _cfgp(config)),
                      "kzgamd_g2_uncompress_batch")
    return out, status.raw[:n], rc


def write_trusted_setup_file(path, g1_monomial, g1_lagrange, g2_monomial, num_g1, num_g2, config=None):
    """a setup of any size as text in the layout load_trusted_setup_file reads; the points are compressed on the GPU"""
    f = _fopen(path, b"w")
    try:
        rc = lib().kzgamd_write_trusted_setup_file(f, _addr(g1_monomial) if num_g1 else None, _addr(g1_lagrange) if num_g1 else None,
                                                   _addr(g2_monomial) if num_g2 else None, num_g1, num_g2, _cfgp(config))
    finally:
        _libc.fclose(f)
    if rc != 0:
        raise KzgAmdError("kzgamd_write_trusted_setup_file: %d" % rc)


def read_trusted_setup_file(path, config=None, capacity=None):
    """(g1_monomial, g1_lagrange, g2_monomial, num_g1, num_g2, rc) of a setup file of any size, parsed on the GPU with
    the subgroup test: rc 0 ok, 1 malformed text, 2 `capacity` = (g1, g2) too small, 3 a point was refused (all-zero).
    capacity None: the counts are read first and the arrays sized by them."""
    def call(mono, lag, g2, cap):
        n1, n2 = C.c_size_t(cap[0]), C.c_size_t(cap[1])
        f = _fopen(path)
        try:
            rc = lib().kzgamd_read_trusted_setup_file(f, mono, lag, g2, C.byref(n1), C.byref(n2), _cfgp(config))
        finally:
            _libc.fclose(f)
        if rc < 0:
            raise KzgAmdError("kzgamd_read_trusted_setup_file: %d" % rc)
        return n1.value, n2.value, rc

    if capacity is None:
        n1, n2, rc = call(None, None, None, (0, 0))
        if rc != 0:
            return None, None, None, n1, n2, rc
        capacity = (n1, n2)
    mono, lag, g2 = (BlstP1 * max(capacity[0], 1))(), (BlstP1 * max(capacity[0], 1))(), (BlstP2 * max(capacity[1], 1))()
    n1, n2, rc = call(mono, lag, g2, capacity)
    return mono, lag, g2, n1, n2, rc


def g2_lincomb(points, scalars, n, config=None):
    """sum_i scalars[i] * points[i] on the GPU: BlstP2[n] (any Z) and Montgomery blst_fr[n]; returns a new BlstP2
    (all-zero for the identity, which is also what n = 0 gives)"""
    out = BlstP2()
    rc = lib().kzgamd_g2_lincomb(C.byref(out), _addr(points) if n else None, _addr(scalars) if n else None, n, _cfgp(config))
    if rc != 0:
        raise KzgAmdError("kzgamd_g2_lincomb: %d" % rc)
    return out


def g2_lincomb_info() -> int:
    """the points one slice of g2_lincomb takes"""
    out = C.c_size_t(0)
    lib().kzgamd_g2_lincomb_info(C.byref(out))
    return out.value


class G2Msm:
    """A prepared bucket MSM in G2 (kzgamd_g2_msm_new): the table 2^(8k) * points[i] of BlstP2[npoints] (any Z) on the
    GPU.  config: the device, table_budget_bytes, and the tuning keys g2msm_segment / g2msm_pass_entries."""

    def __init__(self, points, npoints, config=None):
        err = C.c_int(0)
        self.npoints = npoints
        self.handle = lib().kzgamd_g2_msm_new(_addr(points) if npoints else None, npoints, _cfgp(config), C.byref(err))
        if not self.handle:
            self.handle = None
            raise KzgAmdError("kzgamd_g2_msm_new: %d" % err.value)

    def g2_msm(self, scalars, n, nbatch=1):
        """BlstP2[nbatch]: out[b] = sum_{i < n} scalars[b * n + i] * points[i] (Montgomery blst_fr[nbatch * n]); every
        output has Z = one, or is all-zero for the identity; nbatch == 0 gives an empty array"""
        out = (BlstP2 * nbatch)()
        rc = lib().kzgamd_g2_msm(self.handle, out if nbatch else None, _addr(scalars) if n and nbatch else None, n, nbatch)
        if rc != 0:
            raise KzgAmdError("kzgamd_g2_msm: %d" % rc)
        return out

    def info(self):
        """the shape of the handle: npoints, window_bits, segment, pass_entries, table_bytes"""
        np_, seg, pe, tb, wb = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        lib().kzgamd_g2_msm_info(self.handle, C.byref(np_), C.byref(wb), C.byref(seg), C.byref(pe), C.byref(tb))
        return {"npoints": np_.value, "window_bits": wb.value, "segment": seg.value, "pass_entries": pe.value, "table_bytes": tb.value}

    def close(self):
        if self.handle:
            lib().kzgamd_g2_msm_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_trusted_setup(g1_monomial, g1_lagrange, g2_monomial, num_g1, num_g2, fft_settings=None, seed=None, config=None):
    """(rc, failed) of kzgamd_verify_trusted_setup: rc 0 the setup passed, 1 it did not and `failed` has the bits of the
    checks that failed (1 generators, 2 G1 powers, 4 G2 powers, 8 Lagrange form), 2 fewer than two points on a side,
    3 the Lagrange form cannot be checked (no FFTSettings, not a power of two, too wide).  g1_lagrange None: that check
    is not made.  seed: 32 bytes the maker of the setup could not know, or None (a hash of the setup itself)."""
    if seed is not None and len(seed) != 32:
        raise KzgAmdError("verify_trusted_setup: the seed is 32 bytes")
    failed = C.c_uint(0)
    rc = lib().kzgamd_verify_trusted_setup(fft_settings.handle if fft_settings is not None else None, C.byref(failed), _addr(g1_monomial),
                                           _addr(g1_lagrange) if g1_lagrange is not None else None, _addr(g2_monomial), num_g1, num_g2,
                                           bytes(seed) if seed is not None else None, _cfgp(config))
    if rc < 0:
        raise KzgAmdError("kzgamd_verify_trusted_setup: %d" % rc)
    return rc, failed.value


def verify_trusted_setup_file(path, fft_settings, seed=None, config=None):
    """(rc, failed) of kzgamd_verify_trusted_setup_file: as verify_trusted_setup, and 11, 12, 13 for what the reader
    refuses (malformed text, -, a refused point)"""
    failed = C.c_uint(0)
    f = _fopen(path)
    try:
        rc = lib().kzgamd_verify_trusted_setup_file(fft_settings.handle if fft_settings is not None else None, C.byref(failed), f,
                                                    bytes(seed) if seed is not None else None, _cfgp(config))
    finally:
        _libc.fclose(f)
    if rc < 0:
        raise KzgAmdError("kzgamd_verify_trusted_setup_file: %d" % rc)
    return rc, failed.value


def p2_in_g2(p) -> bool:
    """the subgroup test of one BlstP2 on the host (psi(P) == [x]P)"""
    return lib().kzgamd_p2_in_g2(C.byref(p)) == 1


def codec_info() -> int:
    """the points one slice of the batched codec calls takes"""
    out = C.c_size_t(0)
    lib().kzgamd_codec_info(C.byref(out))
    return out.value


def compute_challenge(blob: bytes, commitment_p1) -> BlstFr:
    """blst/src/eip_4844.rs:501-514 (commitment: BlstP1)"""
    out = BlstFr()
    lib().compute_challenge(C.byref(out), blob, C.byref(commitment_p1))
    return out


def bytes_to_kzg_commitment(b: bytes) -> BlstP1:
    out = BlstP1()
    if len(b) != 48 or lib().bytes_to_kzg_commitment(C.byref(out), b) != C_KZG_OK:
        raise KzgAmdError("bytes_to_kzg_commitment: C_KZG_RET %d" % C_KZG_BADARGS)
    return out


def bytes_from_bls_field(fr) -> bytes:
    out = C.create_string_buffer(32)
    lib().bytes_from_bls_field(out, C.byref(fr))
    return out.raw


def compute_cells_and_kzg_proofs(blob: bytes, settings: KZGSettings, want_cells=True, want_proofs=True):
    """kzg/src/eth/c_bindings.rs:356-372 -> (cells bytes 128*2048 | None, proofs bytes 128*48 | None)"""
    if len(blob) != BYTES_PER_BLOB:
        raise KzgAmdError("compute_cells_and_kzg_proofs: C_KZG_RET %d" % C_KZG_BADARGS)
    cells = C.create_string_buffer(128 * 2048) if want_cells else None
    proofs = C.create_string_buffer(128 * 48) if want_proofs else None
    rc = lib().compute_cells_and_kzg_proofs(cells, proofs, blob, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("compute_cells_and_kzg_proofs: C_KZG_RET %d" % rc)
    return (cells.raw if cells else None), (proofs.raw if proofs else None)


def recover_cells_and_kzg_proofs(cell_indices, cells: bytes, settings: KZGSettings, want_proofs=True):
    """kzg/src/eth/c_bindings.rs:202-289 -> (cells bytes 128*2048, proofs bytes 128*48 | None)"""
    n = len(cell_indices)
    idx = (C.c_uint64 * max(n, 1))(*cell_indices)
    out_cells = C.create_string_buffer(128 * 2048)
    out_proofs = C.create_string_buffer(128 * 48) if want_proofs else None
    f = lib().recover_cells_and_kzg_proofs
    f.restype = C.c_int
    rc = f(out_cells, out_proofs, idx, cells, C.c_uint64(n), C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("recover_cells_and_kzg_proofs: C_KZG_RET %d" % rc)
    return out_cells.raw, (out_proofs.raw if out_proofs else None)


def recover_cells_and_kzg_proofs_batch(indices_per_blob, cells_per_blob, settings: KZGSettings, want_proofs=True):
    """kzgamd_recover_cells_and_kzg_proofs_batch (das.rs:209-241): blob b gives the cells cells_per_blob[b] (bytes,
    2048 per cell) at the indices indices_per_blob[b] -> (list of n cells bytes 128*2048, list of n proofs bytes 128*48
    | None), what n calls of recover_cells_and_kzg_proofs give"""
    n = len(indices_per_blob)
    counts = [len(ix) for ix in indices_per_blob]
    if len(cells_per_blob) != n or any(len(c) != 2048 * k for c, k in zip(cells_per_blob, counts)):
        # cells that do not match their indices cannot be expressed through (pointer, num_cells)
        raise KzgAmdError("kzgamd_recover_cells_and_kzg_proofs_batch: C_KZG_RET %d" % C_KZG_BADARGS)
    flat = [i for ix in indices_per_blob for i in ix]
    idx = (C.c_uint64 * max(len(flat), 1))(*flat)
    num = (C.c_uint64 * max(n, 1))(*counts)
    cells = b"".join(cells_per_blob)
    out_cells = C.create_string_buffer(max(n, 1) * 128 * 2048)
    out_proofs = C.create_string_buffer(max(n, 1) * 128 * 48) if want_proofs else None
    rc = lib().kzgamd_recover_cells_and_kzg_proofs_batch(out_cells, out_proofs, idx, cells, num, n, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_recover_cells_and_kzg_proofs_batch: C_KZG_RET %d" % rc)
    raw = out_cells.raw
    got = [raw[b * 262144:(b + 1) * 262144] for b in range(n)]
    if not want_proofs:
        return got, None
    raw = out_proofs.raw
    return got, [raw[b * 6144:(b + 1) * 6144] for b in range(n)]


def verify_cell_kzg_proof_batch(commitments: bytes, cell_indices, cells: bytes, proofs: bytes, settings: KZGSettings):
    """kzg/src/eth/c_bindings.rs:290-355 -> bool; len(cell_indices) tuples of 48 + 2048 + 48 bytes"""
    n = len(cell_indices)
    idx = (C.c_uint64 * max(n, 1))(*cell_indices)
    ok = C.c_bool(False)
    f = lib().verify_cell_kzg_proof_batch
    f.restype = C.c_int
    rc = f(C.byref(ok), commitments, idx, cells, proofs, C.c_uint64(n), C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("verify_cell_kzg_proof_batch: C_KZG_RET %d" % rc)
    return bool(ok.value)


def _vcells_many_args(batches):
    """batches: a list of (commitments bytes, cell_indices, cells bytes, proofs bytes), one per batch, as
    verify_cell_kzg_proof_batch takes them -> the concatenated arrays of the C call"""
    counts = [len(b[1]) for b in batches]
    if any(len(b[0]) != 48 * k or len(b[2]) != 2048 * k or len(b[3]) != 48 * k for b, k in zip(batches, counts)):
        # arrays that do not match their indices cannot be expressed through (pointer, num_cells)
        raise KzgAmdError("kzgamd_verify_cell_kzg_proof_batch_many: C_KZG_RET %d" % C_KZG_BADARGS)
    flat = [i for b in batches for i in b[1]]
    idx = (C.c_uint64 * max(len(flat), 1))(*flat)
    num = (C.c_uint64 * max(len(batches), 1))(*counts)
    return b"".join(b[0] for b in batches), idx, b"".join(b[2] for b in batches), b"".join(b[3] for b in batches), num


def verify_cell_kzg_proof_batch_many(batches, settings: KZGSettings, rho=None, want_each=True):
    """kzgamd_verify_cell_kzg_proof_batch_many: len(batches) verify_cell_kzg_proof_batch inputs (tuples of commitments
    bytes, cell_indices, cells bytes, proofs bytes) under one pairing -> (ok, ok_each): ok_each[b] is the single call's
    verdict for batch b (None with want_each=False), ok their conjunction.  rho (a BlstFr, Montgomery; None: derived
    from the batches' own challenges) must be fixed after every input is."""
    coms, idx, cells, proofs, num = _vcells_many_args(batches)
    n = len(batches)
    ok = C.c_bool(False)
    per = (C.c_bool * max(1, n))() if want_each else None
    rc = lib().kzgamd_verify_cell_kzg_proof_batch_many(C.byref(ok), per, coms, idx, cells, proofs, num, n, _one_fr(rho),
                                                       C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_verify_cell_kzg_proof_batch_many: C_KZG_RET %d" % rc)
    return bool(ok.value), ([bool(per[b]) for b in range(n)] if want_each else None)


def verify_cell_kzg_proof_batch_many_g1(batches, settings: KZGSettings, rho=None):
    """The two G1 sides of verify_cell_kzg_proof_batch_many, no pairing: (BlstP1 * 2) = P, L with
    e(L, G2) == e(P, g2_values_monomial[64]) the verdict"""
    coms, idx, cells, proofs, num = _vcells_many_args(batches)
    out = (BlstP1 * 2)()
    rc = lib().kzgamd_verify_cell_kzg_proof_batch_many_g1(out, coms, idx, cells, proofs, num, len(batches), _one_fr(rho),
                                                          C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_verify_cell_kzg_proof_batch_many_g1: C_KZG_RET %d" % rc)
    return out


def vcells_info() -> int:
    """kzgamd_vcells_info: the cells one wave of the aggregation kernel sums (the slice length a column is cut into)"""
    out = C.c_size_t(0)
    lib().kzgamd_vcells_info(C.byref(out))
    return out.value


VCELLS_STAGES = ("prepare", "upload", "hash", "scalars", "aggregate", "msm", "pairing", "fallback")


def vcells_timing(settings: KZGSettings):
    """kzgamd_vcells_timing: {stage: host ms} of the last verify_cell_kzg_proof_batch_many(_g1) call on `settings`"""
    ms = (C.c_double * 8)()
    if lib().kzgamd_vcells_timing(C.byref(settings.c), ms) != 0:
        raise KzgAmdError("kzgamd_vcells_timing")
    return dict(zip(VCELLS_STAGES, ms))


def compute_verify_cell_kzg_proof_batch_challenge(commitments: bytes, commitment_indices, cell_indices, cells: bytes, proofs: bytes):
    """blst/src/eip_7594.rs:35-97 -> the challenge as 32 big-endian bytes (canonical)"""
    n = len(cell_indices)
    ci = (C.c_uint64 * max(n, 1))(*commitment_indices)
    idx = (C.c_uint64 * max(n, 1))(*cell_indices)
    out = BlstFr()
    f = lib().compute_verify_cell_kzg_proof_batch_challenge
    f.restype = C.c_int
    rc = f(C.byref(out), commitments, C.c_uint64(len(commitments) // 48), ci, idx, cells, proofs, C.c_uint64(n))
    if rc != C_KZG_OK:
        raise KzgAmdError("compute_verify_cell_kzg_proof_batch_challenge: C_KZG_RET %d" % rc)
    b = C.create_string_buffer(32)
    lib().bytes_from_bls_field(b, C.byref(out))
    return b.raw


def compute_cells_and_kzg_proofs_batch(blobs: bytes, n: int, settings: KZGSettings):
    cells = C.create_string_buffer(n * 128 * 2048)
    proofs = C.create_string_buffer(n * 128 * 48)
    rc = lib().kzgamd_compute_cells_and_kzg_proofs_batch(cells, proofs, blobs, n, C.byref(settings.c))
    if rc != C_KZG_OK:
        raise KzgAmdError("kzgamd_compute_cells_and_kzg_proofs_batch: C_KZG_RET %d" % rc)
    return cells.raw, proofs.raw


# ---------------------------------------------------------------- multi-GPU inside the library (csrc/multi.hip)
class MultiKZGSettings:
    """ndev CKZGSettings objects of one trusted setup, one per entry of `devices` (kzgamd_load_trusted_setup_file_multi):
    the in-process multi-GPU path — contiguous slabs of blobs per settings object, one host thread each, inside the
    library.  Two entries may name the same GPU (how the path is tested on a one-GPU box)."""

    def __init__(self, path, devices, config=None):
        self.ndev = len(devices)
        self.devices = list(devices)
        self.arr = (CKZGSettings * self.ndev)()
        self.loaded = False
        devs = (C.c_int * self.ndev)(*self.devices)
        f = _fopen(path)
        try:
            rc = lib().kzgamd_load_trusted_setup_file_multi_ex(self.arr, devs, self.ndev, f, _cfgp(config)) if config is not None \
                else lib().kzgamd_load_trusted_setup_file_multi(self.arr, devs, self.ndev, f)
        finally:
            _libc.fclose(f)
        if rc != C_KZG_OK:
            raise KzgAmdError("kzgamd_load_trusted_setup_file_multi: C_KZG_RET %d" % rc)
        self.loaded = True
        self.ptrs = (C.POINTER(CKZGSettings) * self.ndev)(*[C.pointer(self.arr[d]) for d in range(self.ndev)])

    def settings_devices(self):
        return [lib().kzgamd_settings_device(C.byref(self.arr[d])) for d in range(self.ndev)]

    def table_info(self, d, which=0):
        c, rows, wide = C.c_int(), C.c_int(), C.c_int()
        rc = lib().kzgamd_settings_table_info(C.byref(self.arr[d]), which, C.byref(c), C.byref(rows), C.byref(wide))
        return {"rc": rc, "window_bits": c.value, "rows": rows.value, "wide_table": wide.value}

    def commit_batch(self, blobs: bytes, n: int):
        out = C.create_string_buffer(48 * max(n, 1))
        rc = lib().kzgamd_blob_to_kzg_commitment_batch_multi(out, blobs, n, self.ptrs, self.ndev)
        if rc != C_KZG_OK:
            raise KzgAmdError("kzgamd_blob_to_kzg_commitment_batch_multi: C_KZG_RET %d" % rc)
        raw = out.raw
        return [raw[48 * i:48 * i + 48] for i in range(n)]

    def proof_batch(self, blobs: bytes, commitments: bytes, n: int):
        out = C.create_string_buffer(48 * max(n, 1))
        rc = lib().kzgamd_compute_blob_kzg_proof_batch_multi(out, blobs, commitments, n, self.ptrs, self.ndev)
        if rc != C_KZG_OK:
            raise KzgAmdError("kzgamd_compute_blob_kzg_proof_batch_multi: C_KZG_RET %d" % rc)
        raw = out.raw
        return [raw[48 * i:48 * i + 48] for i in range(n)]

    def cells_and_proofs_batch(self, blobs: bytes, n: int):
        cells = C.create_string_buffer(max(n, 1) * 128 * 2048)
        proofs = C.create_string_buffer(max(n, 1) * 128 * 48)
        rc = lib().kzgamd_compute_cells_and_kzg_proofs_batch_multi(cells, proofs, blobs, n, self.ptrs, self.ndev)
        if rc != C_KZG_OK:
            raise KzgAmdError("kzgamd_compute_cells_and_kzg_proofs_batch_multi: C_KZG_RET %d" % rc)
        return cells.raw[:n * 128 * 2048], proofs.raw[:n * 128 * 48]

    def verify_blob_batch(self, blobs: bytes, commitments: bytes, proofs: bytes, n: int) -> bool:
        ok = C.c_bool(False)
        return _verdict(lib().kzgamd_verify_blob_kzg_proof_batch_multi(C.byref(ok), blobs, commitments, proofs, n, self.ptrs,
                                                                       self.ndev), ok, "kzgamd_verify_blob_kzg_proof_batch_multi")

    def close(self):
        if self.loaded:
            lib().kzgamd_free_trusted_setup_multi(self.arr, self.ndev)
            self.loaded = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mult_pippenger_prepared_multi(handles, offsets, scalars):
    """kzgamd_mult_pippenger_prepared_multi: handles[d] prepared over points[offsets[d]:offsets[d+1]]; returns BlstP1."""
    nd = len(handles)
    hs = (C.c_void_p * nd)(*[h.handle for h in handles])
    offs = (C.c_size_t * (nd + 1))(*offsets)
    out = BlstP1()
    _check(lib().kzgamd_mult_pippenger_prepared_multi(hs, nd, C.byref(out), offs, _addr(scalars)),
           "kzgamd_mult_pippenger_prepared_multi")
    return out
