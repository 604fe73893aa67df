//! FFI to libkzg_mi355x.so (include/kzg_mi355x.h) and the thin safe layer `rust-kzg-blst` would call.
//!
//! NOT COMPILED in the build image (no rustc/cargo there); every behaviour that matters is implemented
//! and tested on the C side of this boundary.  Mapping to the reference:
//!   * `GpuMsm` / `msm_prepared` / `msm`  <->  blst-sppark/src/lib.rs:8-62 (same three C symbols)
//!   * `GpuNtt::fft_fr` / `das_fft_extension` / `fft_g1`  <->  blst/src/fft_fr.rs:156-165,
//!     blst/src/data_availability_sampling.rs:78-100, blst/src/fft_g1.rs:54-83
//!   * `g1_sum`  —  combine step of one MSM split over several GPUs
use blst::{blst_fr, blst_p1, blst_p1_affine, blst_p2};
use core::ffi::{c_char, c_int, c_void};

#[repr(C)]
pub struct RustError {
    pub code: c_int,
    pub message: *mut c_char,
}

/// `KzgAmdConfig` of include/kzg_mi355x.h: device, HBM budget per fixed-base table, tuning string.
#[repr(C)]
pub struct KzgAmdConfig {
    pub struct_size: u32,
    pub device: i32,
    pub table_budget_bytes: u64,
    pub tuning: *const c_char,
}

impl Default for KzgAmdConfig {
    fn default() -> Self {
        let mut cfg = core::mem::MaybeUninit::<KzgAmdConfig>::uninit();
        unsafe {
            kzgamd_config_init(cfg.as_mut_ptr());
            cfg.assume_init()
        }
    }
}

extern "C" {
    fn kzgamd_config_init(cfg: *mut KzgAmdConfig);
    fn kzgamd_prepare_msm_ex(points: *const blst_p1_affine, npoints: usize, cfg: *const KzgAmdConfig) -> *mut c_void;
    fn kzgamd_prepare_msm_matrix(points: *const blst_p1_affine, rows: usize, cols: usize, cfg: *const KzgAmdConfig) -> *mut c_void;
    fn kzgamd_msm_attach_matrix(msm: *mut c_void, points: *const blst_p1_affine, rows: usize, cols: usize,
                                cfg: *const KzgAmdConfig) -> RustError;
    fn kzgamd_mult_pippenger_matrix(msm: *mut c_void, out: *mut blst_p1, scalars: *const blst_fr, nmat: usize) -> RustError;
    fn kzgamd_msm_matrix_shape(msm: *mut c_void, rows: *mut usize, cols: *mut usize) -> c_int;
    fn kzgamd_ntt_new_ex(scale: u32, cfg: *const KzgAmdConfig) -> *mut c_void;
    fn prepare_msm(points: *const blst_p1_affine, npoints: usize) -> *mut c_void;
    fn free_msm(msm: *mut c_void);
    fn mult_pippenger_prepared(msm: *mut c_void, out: *mut blst_p1, npoints: usize, scalars: *const blst_fr) -> RustError;
    fn mult_pippenger_prepared_batch(msm: *mut c_void, out: *mut blst_p1, npoints: usize, nbatch: usize,
                                     scalars: *const blst_fr) -> RustError;
    fn mult_pippenger(out: *mut blst_p1, points: *const blst_p1_affine, npoints: usize, scalars: *const blst_fr) -> RustError;

    fn kzgamd_ntt_new(scale: u32) -> *mut c_void;
    fn kzgamd_ntt_free(ctx: *mut c_void);
    fn ntt_fr(ctx: *mut c_void, out: *mut blst_fr, input: *const blst_fr, n: usize, inverse: c_int) -> c_int;
    fn das_fft_extension(ctx: *mut c_void, odds: *mut blst_fr, evens: *const blst_fr, half_n: usize) -> c_int;
    fn fft_g1(ctx: *mut c_void, out: *mut blst_p1, input: *const blst_p1, n: usize, inverse: c_int) -> c_int;
    fn kzgamd_g1_sum(out: *mut blst_p1, input: *const blst_p1, n: usize);

    fn kzgamd_fk20_new(ntt: *mut c_void, g1_monomial: *const blst_p1, num_g1: usize, n2: usize, chunk_len: usize,
                       cfg: *const KzgAmdConfig, err: *mut c_int) -> *mut c_void;
    fn kzgamd_fk20_free(fk: *mut c_void);
    fn kzgamd_fk20_da(fk: *mut c_void, out: *mut blst_p1, polys: *const blst_fr, n: usize, npoly: usize,
                      optimized: c_int) -> c_int;
    fn kzgamd_fk20_info(fk: *mut c_void, n2: *mut usize, chunk_len: *mut usize, form: *mut c_int) -> c_int;

    fn kzgamd_kzg_new(ntt: *mut c_void, g1_monomial: *const blst_p1, num_g1: usize, g2_monomial: *const blst_p2, num_g2: usize,
                      cfg: *const KzgAmdConfig, err: *mut c_int) -> *mut c_void;
    fn kzgamd_kzg_free(kz: *mut c_void);
    fn kzgamd_kzg_info(kz: *mut c_void, num_g1: *mut usize, num_g2: *mut usize, chunk: *mut usize,
                       lane_form_min: *mut usize) -> c_int;
    fn kzgamd_kzg_commit(kz: *mut c_void, out: *mut blst_p1, polys: *const blst_fr, len: usize, npoly: usize) -> c_int;
    fn kzgamd_kzg_open(kz: *mut c_void, proofs: *mut blst_p1, ys: *mut blst_fr, polys: *const blst_fr, len: usize,
                       npoly: usize, xs: *const blst_fr, nx: usize, n: usize) -> c_int;
    fn kzgamd_kzg_check(kz: *mut c_void, ok: *mut bool, commitments: *const blst_p1, proofs: *const blst_p1,
                        xs: *const blst_fr, ys: *const blst_fr, n: usize, count: usize) -> c_int;
    fn kzgamd_kzg_check_batch(kz: *mut c_void, ok: *mut bool, ok_each: *mut bool, commitments: *const blst_p1,
                              proofs: *const blst_p1, xs: *const blst_fr, ys: *const blst_fr, n: usize, count: usize,
                              r: *const blst_fr) -> c_int;
    fn kzgamd_kzg_check_batch_g1(kz: *mut c_void, out: *mut blst_p1, commitments: *const blst_p1, proofs: *const blst_p1,
                                 xs: *const blst_fr, ys: *const blst_fr, n: usize, count: usize, r: *const blst_fr) -> c_int;
    fn kzgamd_kzg_batch_challenge(r_out: *mut blst_fr, commitments: *const blst_p1, proofs: *const blst_p1,
                                  xs: *const blst_fr, ys: *const blst_fr, n: usize, count: usize) -> c_int;

    fn kzgamd_poly_new(ntt: *mut c_void, cfg: *const KzgAmdConfig, err: *mut c_int) -> *mut c_void;
    fn kzgamd_poly_free(ph: *mut c_void);
    fn kzgamd_poly_info(ph: *mut c_void, max_width: *mut usize, eval_chunk: *mut usize, mul_direct_max: *mut usize,
                        inv_direct_max: *mut usize) -> c_int;
    fn kzgamd_poly_eval(ph: *mut c_void, ys: *mut blst_fr, polys: *const blst_fr, len: usize, npoly: usize,
                        xs: *const blst_fr, nx: usize) -> c_int;
    fn kzgamd_poly_scale(ph: *mut c_void, out: *mut blst_fr, input: *const blst_fr, len: usize, npoly: usize,
                         inverse: c_int) -> c_int;
    fn kzgamd_poly_mul(ph: *mut c_void, out: *mut blst_fr, a: *const blst_fr, la: usize, b: *const blst_fr, lb: usize,
                       out_len: usize, npoly: usize, form: c_int) -> c_int;
    fn kzgamd_poly_inverse(ph: *mut c_void, out: *mut blst_fr, b: *const blst_fr, lb: usize, out_len: usize,
                           npoly: usize) -> c_int;
    fn kzgamd_poly_div(ph: *mut c_void, q: *mut blst_fr, a: *const blst_fr, la: usize, b: *const blst_fr, lb: usize,
                       npoly: usize) -> c_int;
    fn kzgamd_poly_transform_len(op: c_int, la: usize, lb: usize, out_len: usize) -> usize;
    fn kzgamd_poly_zero_partial(ph: *mut c_void, out: *mut blst_fr, idxs: *const u64, nidx: usize, stride: usize) -> c_int;
    fn kzgamd_poly_reduce_partials(ph: *mut c_void, out: *mut blst_fr, domain_size: usize, partials: *const blst_fr,
                                   lens: *const usize, npartial: usize) -> c_int;
    fn kzgamd_poly_zero_poly(ph: *mut c_void, zero_eval: *mut blst_fr, zero_poly: *mut blst_fr, domain_size: usize,
                             missing: *const u64, offsets: *const usize, nprob: usize, form: c_int) -> c_int;
    fn kzgamd_poly_recover(ph: *mut c_void, out: *mut blst_fr, samples: *const blst_fr, present: *const u8, n: usize,
                           nprob: usize, coeffs: c_int) -> c_int;
    fn kzgamd_poly_zero_info(ph: *mut c_void, leaf_roots: *mut usize, direct_max: *mut usize) -> c_int;
    fn kzgamd_poly_zero_plan(count: usize, levels: *mut usize) -> usize;

    fn kzgamd_g1_mul_batch(out: *mut blst_p1, base: *const blst_p1, scalars: *const blst_fr, n: usize,
                           cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_g2_mul_batch(out: *mut blst_p2, base: *const blst_p2, scalars: *const blst_fr, n: usize,
                           cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_generate_trusted_setup(ntt: *mut c_void, g1_monomial: *mut blst_p1, g1_lagrange: *mut blst_p1,
                                     g2_monomial: *mut blst_p2, num_g1: usize, num_g2: usize, secret: *const u8,
                                     cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_group_mul_info(slice_points: *mut usize, g1_window_bits: *mut c_int, g2_window_bits: *mut c_int) -> c_int;

    pub fn kzgamd_g2_msm_new(points: *const blst_p2, npoints: usize, cfg: *const KzgAmdConfig, err: *mut c_int) -> *mut c_void;
    pub fn kzgamd_g2_msm_free(h: *mut c_void);
    pub fn kzgamd_g2_msm(h: *mut c_void, out: *mut blst_p2, scalars: *const blst_fr, n: usize, nbatch: usize) -> c_int;
    pub fn kzgamd_g2_msm_info(h: *mut c_void, npoints: *mut usize, window_bits: *mut c_int, segment: *mut usize,
                              pass_entries: *mut usize, table_bytes: *mut usize) -> c_int;

    fn kzgamd_g1_compress_batch(out48: *mut u8, points: *const blst_p1, n: usize, cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_g1_to_affine_batch(out: *mut blst_p1_affine, points: *const blst_p1, n: usize, cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_g1_uncompress_batch(out: *mut blst_p1, status: *mut u8, in48: *const u8, n: usize, check_subgroup: c_int,
                                  cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_g2_compress_batch(out96: *mut u8, points: *const blst_p2, n: usize, cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_g2_uncompress_batch(out: *mut blst_p2, status: *mut u8, in96: *const u8, n: usize, check_subgroup: c_int,
                                  cfg: *const KzgAmdConfig) -> c_int;
    fn kzgamd_p2_in_g2(p: *const blst_p2) -> c_int;
    fn kzgamd_codec_info(slice_points: *mut usize) -> c_int;
    /// `out` / `input` are C `FILE *` streams (e.g. from `libc::fopen` / `libc::fdopen`).
    pub fn kzgamd_write_trusted_setup_file(out: *mut c_void, g1_monomial: *const blst_p1, g1_lagrange: *const blst_p1,
                                           g2_monomial: *const blst_p2, num_g1: usize, num_g2: usize,
                                           cfg: *const KzgAmdConfig) -> c_int;
    pub fn kzgamd_read_trusted_setup_file(input: *mut c_void, g1_monomial: *mut blst_p1, g1_lagrange: *mut blst_p1,
                                          g2_monomial: *mut blst_p2, num_g1: *mut usize, num_g2: *mut usize,
                                          cfg: *const KzgAmdConfig) -> c_int;
}

fn group_mul_result(rc: c_int, what: &str) -> Result<(), String> {
    match rc {
        0 => Ok(()),
        1 => Err(format!("{what}: the Lagrange form needs an NTT handle and a power-of-two number of G1 points")),
        2 => Err(String::from("Supplied list is longer than the available max width")),
        3 => Err(format!("{what}: the base is not in the G1 subgroup")),
        e => Err(format!("{what}: {e}")),
    }
}

/// `out[i] = scalars[i] * base` on the GPU (`base` None: the generator); scalars in Montgomery form, as `G1Mul::mul`.
pub fn g1_mul_batch(base: Option<&blst_p1>, scalars: &[blst_fr]) -> Result<Vec<blst_p1>, String> {
    let mut out = vec![blst_p1::default(); scalars.len()];
    let b = base.map_or(core::ptr::null(), |p| p as *const blst_p1);
    let rc = unsafe { kzgamd_g1_mul_batch(out.as_mut_ptr(), b, scalars.as_ptr(), scalars.len(), core::ptr::null()) };
    group_mul_result(rc, "kzgamd_g1_mul_batch").map(|_| out)
}

/// The same in G2 (`G2Mul::mul`); the base is not tested for the subgroup.
pub fn g2_mul_batch(base: Option<&blst_p2>, scalars: &[blst_fr]) -> Result<Vec<blst_p2>, String> {
    let mut out = vec![blst_p2::default(); scalars.len()];
    let b = base.map_or(core::ptr::null(), |p| p as *const blst_p2);
    let rc = unsafe { kzgamd_g2_mul_batch(out.as_mut_ptr(), b, scalars.as_ptr(), scalars.len(), core::ptr::null()) };
    group_mul_result(rc, "kzgamd_g2_mul_batch").map(|_| out)
}

/// (outputs per slice of workspace, window bits of the G1 table, of the G2 table)
pub fn group_mul_info() -> (usize, i32, i32) {
    let (mut s, mut a, mut b) = (0usize, 0 as c_int, 0 as c_int);
    unsafe { kzgamd_group_mul_info(&mut s, &mut a, &mut b) };
    (s, a as i32, b as i32)
}

fn codec_result(rc: c_int, what: &str) -> Result<bool, String> {
    match rc {
        0 => Ok(true),
        1 => Ok(false),
        e => Err(format!("{what}: {e}")),
    }
}

/// `G1::to_bytes` for many Jacobian points on the GPU: 48 bytes each.
pub fn g1_compress_batch(points: &[blst_p1]) -> Result<Vec<u8>, String> {
    let mut out = vec![0u8; 48 * points.len()];
    let rc = unsafe { kzgamd_g1_compress_batch(out.as_mut_ptr(), points.as_ptr(), points.len(), core::ptr::null()) };
    codec_result(rc, "kzgamd_g1_compress_batch").map(|_| out)
}

/// `G1Affine::into_affines` on the GPU; the identity is (0, 0).
pub fn g1_to_affine_batch(points: &[blst_p1]) -> Result<Vec<blst_p1_affine>, String> {
    let mut out = vec![blst_p1_affine::default(); points.len()];
    let rc = unsafe { kzgamd_g1_to_affine_batch(out.as_mut_ptr(), points.as_ptr(), points.len(), core::ptr::null()) };
    codec_result(rc, "kzgamd_g1_to_affine_batch").map(|_| out)
}

/// `G1::from_bytes` (and `is_valid`, with `check_subgroup`) for `bytes.len() / 48` points on the GPU: the points, a
/// status per point (0 ok, 1 no valid encoding, 2 outside the subgroup; such entries are all-zero) and "all accepted".
pub fn g1_uncompress_batch(bytes: &[u8], check_subgroup: bool) -> Result<(Vec<blst_p1>, Vec<u8>, bool), String> {
    let n = bytes.len() / 48;
    let (mut out, mut status) = (vec![blst_p1::default(); n], vec![0u8; n]);
    let rc = unsafe {
        kzgamd_g1_uncompress_batch(out.as_mut_ptr(), status.as_mut_ptr(), bytes.as_ptr(), n, check_subgroup as c_int, core::ptr::null())
    };
    codec_result(rc, "kzgamd_g1_uncompress_batch").map(|ok| (out, status, ok))
}

/// `G2::to_bytes` for many Jacobian points on the GPU: 96 bytes each.
pub fn g2_compress_batch(points: &[blst_p2]) -> Result<Vec<u8>, String> {
    let mut out = vec![0u8; 96 * points.len()];
    let rc = unsafe { kzgamd_g2_compress_batch(out.as_mut_ptr(), points.as_ptr(), points.len(), core::ptr::null()) };
    codec_result(rc, "kzgamd_g2_compress_batch").map(|_| out)
}

/// `G2::from_bytes` for `bytes.len() / 96` points on the GPU, as `g1_uncompress_batch`.
pub fn g2_uncompress_batch(bytes: &[u8], check_subgroup: bool) -> Result<(Vec<blst_p2>, Vec<u8>, bool), String> {
    let n = bytes.len() / 96;
    let (mut out, mut status) = (vec![blst_p2::default(); n], vec![0u8; n]);
    let rc = unsafe {
        kzgamd_g2_uncompress_batch(out.as_mut_ptr(), status.as_mut_ptr(), bytes.as_ptr(), n, check_subgroup as c_int, core::ptr::null())
    };
    codec_result(rc, "kzgamd_g2_uncompress_batch").map(|ok| (out, status, ok))
}

/// The subgroup test of one G2 point on the host.
pub fn p2_in_g2(p: &blst_p2) -> bool {
    unsafe { kzgamd_p2_in_g2(p) == 1 }
}

/// Points per slice of workspace of the batched codec calls.
pub fn codec_info() -> usize {
    let mut s = 0usize;
    unsafe { kzgamd_codec_info(&mut s) };
    s
}

fn check(err: RustError, what: &str) -> Result<(), String> {
    if err.code == 0 {
        return Ok(());
    }
    let msg = if err.message.is_null() {
        format!("{what}: error {}", err.code)
    } else {
        // the library malloc()s the message; take a copy and release it
        let s = unsafe { std::ffi::CStr::from_ptr(err.message) }.to_string_lossy().into_owned();
        unsafe { libc_free(err.message as *mut c_void) };
        format!("{what}: {s}")
    };
    Err(msg)
}

extern "C" {
    #[link_name = "free"]
    fn libc_free(p: *mut c_void);
}

/// Owning handle over the device-resident fixed-base table (what `SpparkPrecomputation.table` points at,
/// kzg/src/msm/sppark.rs:5-22).  Unlike the reference it is released on drop.
pub struct GpuMsm {
    handle: *mut c_void,
    npoints: usize,
}
unsafe impl Send for GpuMsm {}
unsafe impl Sync for GpuMsm {} // calls on one handle serialise inside the library

impl GpuMsm {
    pub fn new(points: &[blst_p1_affine]) -> Result<Self, String> {
        if points.is_empty() {
            return Err("empty point set".into());
        }
        let handle = unsafe { prepare_msm(points.as_ptr(), points.len()) };
        if handle.is_null() {
            return Err("prepare_msm failed (no gfx950 device?)".into());
        }
        Ok(Self { handle, npoints: points.len() })
    }

    /// Sum of scalars[i] * points[i] over the first scalars.len() points; scalars in Montgomery form.
    pub fn msm_prepared(&self, scalars: &[blst_fr]) -> Result<blst_p1, String> {
        if scalars.len() > self.npoints {
            return Err("more scalars than prepared points".into());
        }
        let mut out = blst_p1::default();
        check(unsafe { mult_pippenger_prepared(self.handle, &mut out, scalars.len(), scalars.as_ptr()) },
              "mult_pippenger_prepared")?;
        Ok(out)
    }

    /// `nbatch` MSMs at once; `scalars` is nbatch x npoints, row-major.
    pub fn msm_prepared_batch(&self, scalars: &[blst_fr], npoints: usize) -> Result<Vec<blst_p1>, String> {
        if npoints == 0 || scalars.len() % npoints != 0 || npoints > self.npoints {
            return Err("bad batch shape".into());
        }
        let nbatch = scalars.len() / npoints;
        let mut out = vec![blst_p1::default(); nbatch];
        check(unsafe { mult_pippenger_prepared_batch(self.handle, out.as_mut_ptr(), npoints, nbatch, scalars.as_ptr()) },
              "mult_pippenger_prepared_batch")?;
        Ok(out)
    }
}

/// Raw-handle forms for callers that keep the table behind `kzg::msm::precompute::PrecomputationTable`
/// (an opaque `*mut c_void`, kzg/src/msm/sppark.rs:5-22) instead of a `GpuMsm`.
///
/// # Safety
/// `handle` must come from [`prepare_raw`] (or `GpuMsm`) and not have been freed.
pub unsafe fn msm_prepared_raw(handle: *mut c_void, scalars: &[blst_fr]) -> Result<blst_p1, String> {
    let mut out = blst_p1::default();
    check(mult_pippenger_prepared(handle, &mut out, scalars.len(), scalars.as_ptr()), "mult_pippenger_prepared")?;
    Ok(out)
}

/// # Safety
/// as [`msm_prepared_raw`]; `scalars` is nbatch x npoints, row-major.
pub unsafe fn msm_prepared_batch_raw(handle: *mut c_void, scalars: &[blst_fr], npoints: usize) -> Result<Vec<blst_p1>, String> {
    if npoints == 0 || scalars.len() % npoints != 0 {
        return Err("bad batch shape".into());
    }
    let nbatch = scalars.len() / npoints;
    let mut out = vec![blst_p1::default(); nbatch];
    check(mult_pippenger_prepared_batch(handle, out.as_mut_ptr(), npoints, nbatch, scalars.as_ptr()),
          "mult_pippenger_prepared_batch")?;
    Ok(out)
}

/// The matrix of `precompute(points, matrix)` (kzg/src/msm/bgmw.rs:206-304) attached to a handle of [`prepare_raw`]:
/// `rows` base sets of `cols` points, row-major.  One pointer then serves `g1_lincomb` and `g1_lincomb_batch`.
///
/// # Safety
/// `handle` must come from [`prepare_raw`] and not have been freed.
pub unsafe fn attach_matrix_raw(handle: *mut c_void, points: &[blst_p1_affine], rows: usize, cols: usize,
                                cfg: Option<&KzgAmdConfig>) -> Result<(), String> {
    if rows == 0 || cols == 0 || points.len() != rows * cols {
        return Err("bad matrix shape".into());
    }
    let cfg_ptr = cfg.map_or(core::ptr::null(), |c| c as *const KzgAmdConfig);
    check(kzgamd_msm_attach_matrix(handle, points.as_ptr(), rows, cols, cfg_ptr), "kzgamd_msm_attach_matrix")
}

/// `multiply_batch` (kzg/src/msm/bgmw.rs:306-380) on the attached matrix: `scalars` is rows x cols, row-major;
/// one launch for all rows.
///
/// # Safety
/// `handle` must carry a matrix ([`attach_matrix_raw`]) of `rows` rows.
pub unsafe fn msm_matrix_raw(handle: *mut c_void, scalars: &[blst_fr], rows: usize) -> Result<Vec<blst_p1>, String> {
    let (mut hr, mut hc) = (0usize, 0usize);
    if kzgamd_msm_matrix_shape(handle, &mut hr, &mut hc) != 0 {
        return Err("no matrix attached to this handle".into());
    }
    if rows != hr || scalars.len() != hr * hc {
        return Err("bad matrix shape".into());
    }
    let mut out = vec![blst_p1::default(); rows];
    check(kzgamd_mult_pippenger_matrix(handle, out.as_mut_ptr(), scalars.as_ptr(), 1), "kzgamd_mult_pippenger_matrix")?;
    Ok(out)
}

/// A stand-alone matrix handle (`kzgamd_prepare_msm_matrix`); release with [`free_raw`].
pub fn prepare_matrix_raw(points: &[blst_p1_affine], rows: usize, cols: usize, cfg: Option<&KzgAmdConfig>) -> *mut c_void {
    if rows == 0 || cols == 0 || points.len() != rows * cols {
        return core::ptr::null_mut();
    }
    let cfg_ptr = cfg.map_or(core::ptr::null(), |c| c as *const KzgAmdConfig);
    unsafe { kzgamd_prepare_msm_matrix(points.as_ptr(), rows, cols, cfg_ptr) }
}

/// [`prepare_raw`] with a configuration (device, table budget, tuning).
pub fn prepare_raw_with(points: &[blst_p1_affine], cfg: &KzgAmdConfig) -> *mut c_void {
    unsafe { kzgamd_prepare_msm_ex(points.as_ptr(), points.len(), cfg) }
}

/// `prepare_multi_scalar_mult` of blst-sppark/src/lib.rs:8-17: the handle is leaked into the settings object like
/// the reference's (release it with [`free_raw`] when the settings go away).
pub fn prepare_raw(points: &[blst_p1_affine]) -> *mut c_void {
    unsafe { prepare_msm(points.as_ptr(), points.len()) }
}

/// # Safety
/// `handle` must come from [`prepare_raw`]; it is dead afterwards.
pub unsafe fn free_raw(handle: *mut c_void) {
    free_msm(handle)
}

impl Drop for GpuMsm {
    fn drop(&mut self) {
        unsafe { free_msm(self.handle) }
    }
}

/// Variable-base MSM (the `None` precomputation arm of blst/src/kzg_proofs.rs:53-57).
pub fn msm(points: &[blst_p1_affine], scalars: &[blst_fr]) -> Result<blst_p1, String> {
    if points.len() != scalars.len() {
        return Err("length mismatch".into());
    }
    let mut out = blst_p1::default();
    if points.is_empty() {
        return Ok(out);
    }
    check(unsafe { mult_pippenger(&mut out, points.as_ptr(), points.len(), scalars.as_ptr()) }, "mult_pippenger")?;
    Ok(out)
}

/// Device NTT context; one per `FsFFTSettings` (created in `FFTSettings::new(scale)`).
pub struct GpuNtt {
    ctx: *mut c_void,
}
unsafe impl Send for GpuNtt {}
unsafe impl Sync for GpuNtt {}

impl GpuNtt {
    pub fn new(scale: usize) -> Result<Self, String> {
        if scale >= 32 {
            return Err(String::from("Scale is expected to be within root of unity matrix row size"));
        }
        let ctx = unsafe { kzgamd_ntt_new(scale as u32) };
        if ctx.is_null() {
            return Err("kzgamd_ntt_new failed (no gfx950 device?)".into());
        }
        Ok(Self { ctx })
    }

    /// the same on a chosen device / with tuning keys (`KzgAmdConfig`)
    pub fn with_config(scale: usize, cfg: &KzgAmdConfig) -> Result<Self, String> {
        if scale >= 32 {
            return Err(String::from("Scale is expected to be within root of unity matrix row size"));
        }
        let ctx = unsafe { kzgamd_ntt_new_ex(scale as u32, cfg) };
        if ctx.is_null() {
            return Err("kzgamd_ntt_new_ex failed (no gfx950 device, or a malformed configuration)".into());
        }
        Ok(Self { ctx })
    }

    /// `FFTFr::fft_fr`: natural order in and out, inverse scaled by 1/n; error strings as in the reference.
    pub fn fft_fr(&self, data: &[blst_fr], inverse: bool) -> Result<Vec<blst_fr>, String> {
        let mut out = vec![blst_fr::default(); data.len()];
        match unsafe { ntt_fr(self.ctx, out.as_mut_ptr(), data.as_ptr(), data.len(), inverse as c_int) } {
            0 => Ok(out),
            1 => Err(String::from("Supplied list is longer than the available max width")),
            2 => Err(String::from("A list with power-of-two length expected")),
            e => Err(format!("GPU NTT failed: {e}")),
        }
    }

    /// `FFTG1::fft_g1` (blst/src/fft_g1.rs:54-83); results equal the reference's as group elements.
    pub fn fft_g1(&self, data: &[blst_p1], inverse: bool) -> Result<Vec<blst_p1>, String> {
        let mut out = vec![blst_p1::default(); data.len()];
        match unsafe { fft_g1(self.ctx, out.as_mut_ptr(), data.as_ptr(), data.len(), inverse as c_int) } {
            0 => Ok(out),
            1 => Err(String::from("Supplied list is longer than the available max width")),
            2 => Err(String::from("A list with power-of-two length expected")),
            e => Err(format!("GPU fft_g1 failed: {e}")),
        }
    }

    /// `generate_trusted_setup(n, secret)` of the reference (blst/src/utils.rs:16-37) on the GPU: `[s^i]G1`, their
    /// Lagrange form (the inverse `fft_g1`, natural order) and `[s^i]G2`, `n` of each; `n` a power of two within
    /// this handle's width.
    #[allow(clippy::type_complexity)]
    pub fn generate_trusted_setup(&self, n: usize, secret: &[u8; 32]) -> Result<(Vec<blst_p1>, Vec<blst_p1>, Vec<blst_p2>), String> {
        let mut mono = vec![blst_p1::default(); n];
        let mut lagrange = vec![blst_p1::default(); n];
        let mut g2 = vec![blst_p2::default(); n];
        let rc = unsafe {
            kzgamd_generate_trusted_setup(self.ctx, mono.as_mut_ptr(), lagrange.as_mut_ptr(), g2.as_mut_ptr(), n, n, secret.as_ptr(),
                                          core::ptr::null())
        };
        group_mul_result(rc, "kzgamd_generate_trusted_setup").map(|_| (mono, lagrange, g2))
    }

    /// `DASExtension::das_fft_extension`.
    pub fn das_fft_extension(&self, evens: &[blst_fr]) -> Result<Vec<blst_fr>, String> {
        let mut out = vec![blst_fr::default(); evens.len()];
        match unsafe { das_fft_extension(self.ctx, out.as_mut_ptr(), evens.as_ptr(), evens.len()) } {
            0 => Ok(out),
            1 => Err(String::from("A non-zero list ab expected")),
            2 => Err(String::from("A list with power-of-two length expected")),
            3 => Err(String::from("Supplied list is longer than the available max width")),
            e => Err(format!("GPU DAS extension failed: {e}")),
        }
    }
}

impl Drop for GpuNtt {
    fn drop(&mut self) {
        unsafe { kzgamd_ntt_free(self.ctx) }
    }
}

/// Generic FK20 handle (`kzgamd_fk20_new`): `FK20SingleSettings` (chunk_len = 1) / `FK20MultiSettings` of the reference
/// (blst/src/types/fk20_single_settings.rs, fk20_multi_settings.rs) over a `GpuNtt`.  Holds the NTT handle alive: the
/// C handle keeps it by pointer and must be freed first (field order = drop order).
pub struct GpuFk20 {
    ctx: *mut c_void,
    _ntt: std::sync::Arc<GpuNtt>,
    n2: usize,
    chunk_len: usize,
}
unsafe impl Send for GpuFk20 {}
unsafe impl Sync for GpuFk20 {}

impl GpuFk20 {
    /// Errors carry the reference's messages (fk20_multi_settings.rs:61-73), in the reference's order.
    pub fn new(ntt: std::sync::Arc<GpuNtt>, g1_monomial: &[blst_p1], n2: usize, chunk_len: usize,
               cfg: Option<&KzgAmdConfig>) -> Result<Self, String> {
        let mut err: c_int = 0;
        let cfg_ptr = cfg.map_or(core::ptr::null(), |c| c as *const KzgAmdConfig);
        let ctx = unsafe {
            kzgamd_fk20_new(ntt.ctx, g1_monomial.as_ptr(), g1_monomial.len(), n2, chunk_len, cfg_ptr, &mut err)
        };
        if ctx.is_null() {
            return Err(match err {
                1 => String::from("n2 must be less than or equal to kzg settings max width"),
                2 => String::from("n2 must be a power of two"),
                3 => String::from("n2 must be greater than or equal to 2"),
                4 => String::from("chunk_len must be greater or equal to n2 / 2"),
                5 => String::from("chunk_len must be a power of two"),
                6 => String::from("the setup has fewer than n2 / 2 - chunk_len G1 points"),
                e => format!("kzgamd_fk20_new failed: {e}"),
            });
        }
        Ok(Self { ctx, _ntt: ntt, n2, chunk_len })
    }

    /// `npoly` polynomials of n2 / 2 coefficients each -> npoly * n2 / chunk_len proofs; `optimized`: natural order
    /// (`data_availability_optimized`), else bit-reversed per polynomial (`data_availability`).
    pub fn data_availability(&self, polys: &[blst_fr], npoly: usize, optimized: bool) -> Result<Vec<blst_p1>, String> {
        let n = self.n2 / 2;
        if polys.len() != n * npoly {
            return Err(String::from("n2 must be a power of two"));
        }
        let mut out = vec![blst_p1::default(); npoly * (self.n2 / self.chunk_len)];
        match unsafe { kzgamd_fk20_da(self.ctx, out.as_mut_ptr(), polys.as_ptr(), n, npoly, optimized as c_int) } {
            0 => Ok(out),
            e => Err(format!("GPU FK20 failed: {e}")),
        }
    }

    /// (n2, chunk_len, form): form 1 = a scalar multiplication per product, 2 = wide fixed-base table
    pub fn info(&self) -> (usize, usize, i32) {
        let (mut a, mut b, mut f) = (0usize, 0usize, 0 as c_int);
        unsafe { kzgamd_fk20_info(self.ctx, &mut a, &mut b, &mut f) };
        (a, b, f as i32)
    }
}

impl Drop for GpuFk20 {
    fn drop(&mut self) {
        unsafe { kzgamd_fk20_free(self.ctx) }
    }
}

/// Generic polynomial KZG handle (`kzgamd_kzg_new`): the proving and checking calls of the reference's `KZGSettings`
/// (blst/src/types/kzg_settings.rs:138-277) over a `GpuNtt` and a monomial setup, batched.  Holds the NTT handle alive:
/// the C handle keeps it by pointer and must be freed first (field order = drop order).
pub struct GpuKzg {
    ctx: *mut c_void,
    _ntt: std::sync::Arc<GpuNtt>,
}
unsafe impl Send for GpuKzg {}
unsafe impl Sync for GpuKzg {}

impl core::fmt::Debug for GpuKzg {
    fn fmt(&self, f: &mut core::fmt::Formatter<'_>) -> core::fmt::Result {
        let (num_g1, num_g2, _, _) = self.info();
        write!(f, "GpuKzg {{ num_g1: {num_g1}, num_g2: {num_g2} }}")
    }
}

impl GpuKzg {
    /// `g2_monomial` may be empty: a handle that proves but does not check.
    pub fn new(ntt: std::sync::Arc<GpuNtt>, g1_monomial: &[blst_p1], g2_monomial: &[blst_p2],
               cfg: Option<&KzgAmdConfig>) -> Result<Self, String> {
        let mut err: c_int = 0;
        let cfg_ptr = cfg.map_or(core::ptr::null(), |c| c as *const KzgAmdConfig);
        let g2_ptr = if g2_monomial.is_empty() { core::ptr::null() } else { g2_monomial.as_ptr() };
        let ctx = unsafe {
            kzgamd_kzg_new(ntt.ctx, g1_monomial.as_ptr(), g1_monomial.len(), g2_ptr, g2_monomial.len(), cfg_ptr, &mut err)
        };
        if ctx.is_null() {
            return Err(match err {
                1 => String::from("the setup has no G1 points"),
                e => format!("kzgamd_kzg_new failed: {e}"),
            });
        }
        Ok(Self { ctx, _ntt: ntt })
    }

    /// `commit_to_poly` for `npoly` polynomials of `len` coefficients each (contiguous).
    pub fn commit(&self, polys: &[blst_fr], len: usize, npoly: usize) -> Result<Vec<blst_p1>, String> {
        if polys.len() != len * npoly {
            return Err(String::from("polys must hold npoly * len coefficients"));
        }
        let mut out = vec![blst_p1::default(); npoly];
        match unsafe { kzgamd_kzg_commit(self.ctx, out.as_mut_ptr(), polys.as_ptr(), len, npoly) } {
            0 => Ok(out),
            1 => Err(String::from("Polynomial is longer than secret g1")),
            e => Err(format!("GPU KZG commit failed: {e}")),
        }
    }

    /// `compute_proof_single` (n = 1) / `compute_proof_multi` for every (polynomial, x) pair: npoly * xs.len() proofs,
    /// and with `want_ys` the npoly * xs.len() * n values p(x w^i).
    pub fn open(&self, polys: &[blst_fr], len: usize, npoly: usize, xs: &[blst_fr], n: usize,
                want_ys: bool) -> Result<(Vec<blst_p1>, Vec<blst_fr>), String> {
        if polys.len() != len * npoly {
            return Err(String::from("polys must hold npoly * len coefficients"));
        }
        let pairs = npoly * xs.len();
        let mut proofs = vec![blst_p1::default(); pairs];
        let mut ys = vec![blst_fr::default(); if want_ys { pairs * n } else { 0 }];
        let ys_ptr = if want_ys { ys.as_mut_ptr() } else { core::ptr::null_mut() };
        match unsafe { kzgamd_kzg_open(self.ctx, proofs.as_mut_ptr(), ys_ptr, polys.as_ptr(), len, npoly, xs.as_ptr(), xs.len(), n) } {
            0 => Ok((proofs, ys)),
            1 => Err(String::from("Polynomial is longer than secret g1")),
            2 => Err(String::from("Polynomial must not be empty")),
            3 => Err(String::from("n must be a power of two")),
            4 => Err(String::from("Supplied list is longer than the available max width")),
            e => Err(format!("GPU KZG open failed: {e}")),
        }
    }

    /// `check_proof_single` (n = 1) / `check_proof_multi` for `xs.len()` tuples: one verdict per tuple.
    pub fn check(&self, commitments: &[blst_p1], proofs: &[blst_p1], xs: &[blst_fr], ys: &[blst_fr],
                 n: usize) -> Result<Vec<bool>, String> {
        let count = xs.len();
        if commitments.len() != count || proofs.len() != count || ys.len() != count * n {
            return Err(String::from("commitments, proofs, xs and ys must describe the same number of tuples"));
        }
        let mut ok = vec![false; count];
        match unsafe {
            kzgamd_kzg_check(self.ctx, ok.as_mut_ptr(), commitments.as_ptr(), proofs.as_ptr(), xs.as_ptr(), ys.as_ptr(), n, count)
        } {
            0 => Ok(ok),
            1 => Err(String::from("Polynomial is longer than secret g1")),
            3 => Err(String::from("n is not a power of two")),
            4 => Err(String::from("Supplied list is longer than the available max width")),
            5 => Err(String::from("x must not be zero")),
            6 => Err(String::from("the setup has too few G2 points")),
            e => Err(format!("GPU KZG check failed: {e}")),
        }
    }

    fn batch_error(what: &str, code: c_int) -> String {
        match code {
            1 => String::from("Polynomial is longer than secret g1"),
            3 => String::from("n is not a power of two"),
            4 => String::from("Supplied list is longer than the available max width"),
            5 => String::from("x must not be zero"),
            6 => String::from("the setup has too few G2 points"),
            7 => String::from("a commitment or proof is not on the curve or not in G1"),
            e => format!("GPU KZG {what} failed: {e}"),
        }
    }

    /// All `xs.len()` tuples under ONE pairing (`kzgamd_kzg_check_batch`), weighted by the powers of `r`.  `None`: the
    /// library derives r from the inputs (`batch_challenge`); a caller's own r must be fixed after the inputs are.
    /// With `each` the per-tuple verdicts come back too: all true when the batch passes, `check`'s when it fails.
    pub fn check_batch(&self, commitments: &[blst_p1], proofs: &[blst_p1], xs: &[blst_fr], ys: &[blst_fr], n: usize,
                       r: Option<&blst_fr>, each: bool) -> Result<(bool, Vec<bool>), String> {
        let count = xs.len();
        if commitments.len() != count || proofs.len() != count || ys.len() != count * n {
            return Err(String::from("commitments, proofs, xs and ys must describe the same number of tuples"));
        }
        let mut ok = false;
        let mut per = vec![false; if each { count } else { 0 }];
        let per_ptr = if each { per.as_mut_ptr() } else { core::ptr::null_mut() };
        let r_ptr = r.map_or(core::ptr::null(), |v| v as *const blst_fr);
        match unsafe {
            kzgamd_kzg_check_batch(self.ctx, &mut ok, per_ptr, commitments.as_ptr(), proofs.as_ptr(), xs.as_ptr(), ys.as_ptr(), n,
                                   count, r_ptr)
        } {
            0 => Ok((ok, per)),
            e => Err(Self::batch_error("check_batch", e)),
        }
    }

    /// The two G1 sides of `check_batch`, no pairing: `[L, P]` with e(L, G2) == e(P, [s^n]G2) the verdict.
    pub fn check_batch_g1(&self, commitments: &[blst_p1], proofs: &[blst_p1], xs: &[blst_fr], ys: &[blst_fr], n: usize,
                          r: Option<&blst_fr>) -> Result<[blst_p1; 2], String> {
        let count = xs.len();
        if commitments.len() != count || proofs.len() != count || ys.len() != count * n {
            return Err(String::from("commitments, proofs, xs and ys must describe the same number of tuples"));
        }
        let mut out = [blst_p1::default(); 2];
        let r_ptr = r.map_or(core::ptr::null(), |v| v as *const blst_fr);
        match unsafe {
            kzgamd_kzg_check_batch_g1(self.ctx, out.as_mut_ptr(), commitments.as_ptr(), proofs.as_ptr(), xs.as_ptr(), ys.as_ptr(), n,
                                      count, r_ptr)
        } {
            0 => Ok(out),
            e => Err(Self::batch_error("check_batch_g1", e)),
        }
    }

    /// The weight base `check_batch(r = None)` derives: SHA-256 over the buffers' bytes as passed (host only).
    pub fn batch_challenge(commitments: &[blst_p1], proofs: &[blst_p1], xs: &[blst_fr], ys: &[blst_fr],
                           n: usize) -> Result<blst_fr, String> {
        let count = xs.len();
        if commitments.len() != count || proofs.len() != count || ys.len() != count * n {
            return Err(String::from("commitments, proofs, xs and ys must describe the same number of tuples"));
        }
        let mut r = blst_fr::default();
        match unsafe { kzgamd_kzg_batch_challenge(&mut r, commitments.as_ptr(), proofs.as_ptr(), xs.as_ptr(), ys.as_ptr(), n, count) } {
            0 => Ok(r),
            e => Err(format!("kzgamd_kzg_batch_challenge failed: {e}")),
        }
    }

    /// (num_g1, num_g2, chunk, lane_form_min)
    pub fn info(&self) -> (usize, usize, usize, usize) {
        let (mut a, mut b, mut c, mut d) = (0usize, 0usize, 0usize, 0usize);
        unsafe { kzgamd_kzg_info(self.ctx, &mut a, &mut b, &mut c, &mut d) };
        (a, b, c, d)
    }
}

impl Drop for GpuKzg {
    fn drop(&mut self) {
        unsafe { kzgamd_kzg_free(self.ctx) }
    }
}

/// Batched polynomial arithmetic handle (`kzgamd_poly_new`): the reference's `Poly<Fr>` and `FFTSettingsPoly`
/// (blst/src/types/poly.rs) over a `GpuNtt` — eval, scale / unscale, mul, inverse, div for `npoly` polynomials of one
/// shape per call (contiguous, Montgomery).  Holds the NTT handle alive: the C handle keeps it by pointer and must be
/// freed first (field order = drop order).  Errors carry the reference's messages.
pub struct GpuPoly {
    ctx: *mut c_void,
    _ntt: std::sync::Arc<GpuNtt>,
}
unsafe impl Send for GpuPoly {}
unsafe impl Sync for GpuPoly {} // calls on one handle take turns inside the library

impl core::fmt::Debug for GpuPoly {
    fn fmt(&self, f: &mut core::fmt::Formatter<'_>) -> core::fmt::Result {
        write!(f, "GpuPoly {{ max_width: {} }}", self.info().0)
    }
}

/// Which product `GpuPoly::mul` runs: all give the same elements.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum PolyMulForm {
    Auto = 0,
    Direct = 1,
    Transform = 2,
}

const POLY_TOO_WIDE: &str = "Supplied list is longer than the available max width";

impl GpuPoly {
    pub fn new(ntt: std::sync::Arc<GpuNtt>, cfg: Option<&KzgAmdConfig>) -> Result<Self, String> {
        let mut err: c_int = 0;
        let cfg_ptr = cfg.map_or(core::ptr::null(), |c| c as *const KzgAmdConfig);
        let ctx = unsafe { kzgamd_poly_new(ntt.ctx, cfg_ptr, &mut err) };
        if ctx.is_null() {
            return Err(format!("kzgamd_poly_new failed: {err}"));
        }
        Ok(Self { ctx, _ntt: ntt })
    }

    /// `Poly::eval` of every polynomial at every x: ys[b * xs.len() + k] = p_b(x_k).
    pub fn eval(&self, polys: &[blst_fr], len: usize, npoly: usize, xs: &[blst_fr]) -> Result<Vec<blst_fr>, String> {
        if polys.len() != len * npoly {
            return Err(String::from("polys must hold npoly * len coefficients"));
        }
        let mut ys = vec![blst_fr::default(); npoly * xs.len()];
        match unsafe { kzgamd_poly_eval(self.ctx, ys.as_mut_ptr(), polys.as_ptr(), len, npoly, xs.as_ptr(), xs.len()) } {
            0 => Ok(ys),
            e => Err(format!("GPU poly eval failed: {e}")),
        }
    }

    /// `Poly::scale` (coefficient i times 5^-(i+1)) or, with `inverse`, `Poly::unscale`.
    pub fn scale(&self, polys: &[blst_fr], len: usize, npoly: usize, inverse: bool) -> Result<Vec<blst_fr>, String> {
        if polys.len() != len * npoly {
            return Err(String::from("polys must hold npoly * len coefficients"));
        }
        let mut out = vec![blst_fr::default(); polys.len()];
        match unsafe { kzgamd_poly_scale(self.ctx, out.as_mut_ptr(), polys.as_ptr(), len, npoly, inverse as c_int) } {
            0 => Ok(out),
            e => Err(format!("GPU poly scale failed: {e}")),
        }
    }

    /// The first `out_len` coefficients of a_b * b_b (`Poly::mul`, `mul_direct`, `mul_fft`).
    pub fn mul(&self, a: &[blst_fr], la: usize, b: &[blst_fr], lb: usize, out_len: usize, npoly: usize,
               form: PolyMulForm) -> Result<Vec<blst_fr>, String> {
        if a.len() != la * npoly || b.len() != lb * npoly {
            return Err(String::from("a and b must hold npoly * la and npoly * lb coefficients"));
        }
        let mut out = vec![blst_fr::default(); npoly * out_len];
        match unsafe {
            kzgamd_poly_mul(self.ctx, out.as_mut_ptr(), a.as_ptr(), la, b.as_ptr(), lb, out_len, npoly, form as c_int)
        } {
            0 => Ok(out),
            4 => Err(String::from(POLY_TOO_WIDE)),
            e => Err(format!("GPU poly mul failed: {e}")),
        }
    }

    /// `Poly::inverse`: the first `out_len` coefficients of 1 / b_b as a power series.
    pub fn inverse(&self, b: &[blst_fr], lb: usize, out_len: usize, npoly: usize) -> Result<Vec<blst_fr>, String> {
        if b.len() != lb * npoly {
            return Err(String::from("b must hold npoly * lb coefficients"));
        }
        let mut out = vec![blst_fr::default(); npoly * out_len];
        match unsafe { kzgamd_poly_inverse(self.ctx, out.as_mut_ptr(), b.as_ptr(), lb, out_len, npoly) } {
            0 => Ok(out),
            1 => Err(String::from("Can't produce a zero-length result")),
            2 => Err(String::from("Can't inverse a zero-length poly")),
            3 => Err(String::from("First coefficient of polynomial mustn't be zero")),
            4 => Err(String::from(POLY_TOO_WIDE)),
            e => Err(format!("GPU poly inverse failed: {e}")),
        }
    }

    /// `Poly::div`: npoly quotients of la - lb + 1 coefficients each (none when la < lb).
    pub fn div(&self, a: &[blst_fr], la: usize, b: &[blst_fr], lb: usize, npoly: usize) -> Result<Vec<blst_fr>, String> {
        if a.len() != la * npoly || b.len() != lb * npoly {
            return Err(String::from("a and b must hold npoly * la and npoly * lb coefficients"));
        }
        let qlen = if la >= lb { la - lb + 1 } else { 0 };
        let mut q = vec![blst_fr::default(); npoly * qlen];
        match unsafe { kzgamd_poly_div(self.ctx, q.as_mut_ptr(), a.as_ptr(), la, b.as_ptr(), lb, npoly) } {
            0 => Ok(q),
            1 => Err(String::from("Can't divide by zero")),
            2 => Err(String::from("Highest coefficient must be non-zero")),
            4 => Err(String::from(POLY_TOO_WIDE)),
            e => Err(format!("GPU poly div failed: {e}")),
        }
    }

    /// (max_width, eval_chunk, mul_direct_max, inv_direct_max)
    pub fn info(&self) -> (usize, usize, usize, usize) {
        let (mut a, mut b, mut c, mut d) = (0usize, 0usize, 0usize, 0usize);
        unsafe { kzgamd_poly_info(self.ctx, &mut a, &mut b, &mut c, &mut d) };
        (a, b, c, d)
    }

    /// `do_zero_poly_mul_partial` for any number of indices: the idxs.len() + 1 coefficients of
    /// prod (X - roots[idx * stride]), lowest first.
    pub fn zero_partial(&self, idxs: &[u64], stride: usize) -> Result<Vec<blst_fr>, String> {
        let mut out = vec![blst_fr::default(); idxs.len() + 1];
        match unsafe { kzgamd_poly_zero_partial(self.ctx, out.as_mut_ptr(), idxs.as_ptr(), idxs.len(), stride) } {
            0 => Ok(out),
            1 => Err(String::from("idx array must not be empty")),
            2 => Err(String::from("index out of bounds: idx * stride exceeds max_width")),
            4 => Err(String::from(POLY_TOO_WIDE)),
            e => Err(format!("GPU zero_partial failed: {e}")),
        }
    }

    /// `reduce_partials`: the product of lens.len() polynomials stored back to back in `partials`.
    pub fn reduce_partials(&self, domain_size: usize, partials: &[blst_fr], lens: &[usize]) -> Result<Vec<blst_fr>, String> {
        if partials.len() != lens.iter().sum::<usize>() {
            return Err(String::from("partials must hold the coefficients lens adds up to"));
        }
        let out_len = lens.iter().map(|l| l.saturating_sub(1)).sum::<usize>() + 1;
        let mut out = vec![blst_fr::default(); out_len];
        match unsafe {
            kzgamd_poly_reduce_partials(self.ctx, out.as_mut_ptr(), domain_size, partials.as_ptr(), lens.as_ptr(), lens.len())
        } {
            0 => Ok(out),
            1 => Err(String::from("Expected domain size to be a power of 2")),
            2 => Err(String::from("partials must not be empty")),
            3 => Err(String::from("Out degree is longer than possible polynomial size in domain")),
            4 => Err(String::from("Domain size greater than fft_settings.max_width")),
            5 => Err(String::from("attempt to subtract with overflow: empty partial")),
            e => Err(format!("GPU reduce_partials failed: {e}")),
        }
    }

    /// `zero_poly_via_multiplication` for offsets.len() - 1 index lists in one call (list b is
    /// missing[offsets[b] .. offsets[b + 1]]): (zero_eval, zero_poly), domain_size elements per list each.  An empty
    /// list gives the empty product: the caller that wants the reference's two empty vectors returns them itself.
    pub fn zero_poly(&self, domain_size: usize, missing: &[u64], offsets: &[usize], form: PolyMulForm)
                     -> Result<(Vec<blst_fr>, Vec<blst_fr>), String> {
        if offsets.is_empty() || *offsets.last().unwrap() != missing.len() {
            return Err(String::from("offsets must hold nprob + 1 positions ending at missing.len()"));
        }
        let nprob = offsets.len() - 1;
        let mut ze = vec![blst_fr::default(); nprob * domain_size];
        let mut zp = vec![blst_fr::default(); nprob * domain_size];
        match unsafe {
            kzgamd_poly_zero_poly(self.ctx, ze.as_mut_ptr(), zp.as_mut_ptr(), domain_size, missing.as_ptr(), offsets.as_ptr(),
                                  nprob, form as c_int)
        } {
            0 => Ok((ze, zp)),
            1 => Err(String::from("Missing idxs greater than domain size")),
            2 => Err(String::from("Domain size greater than fft_settings.max_width")),
            3 => Err(String::from("Domain size must be a power of 2")),
            5 => Err(String::from("index out of bounds: missing idx exceeds domain size")),
            e => Err(format!("GPU zero_poly failed: {e}")),
        }
    }

    /// `recover_poly_from_samples` (`coeffs`: `recover_poly_coeffs_from_samples`) for `nprob` vectors of `n` samples;
    /// present[b * n + i] == 0 marks a missing sample, whose value is never used.
    pub fn recover(&self, samples: &[blst_fr], present: &[u8], n: usize, nprob: usize, coeffs: bool) -> Result<Vec<blst_fr>, String> {
        if samples.len() != n * nprob || present.len() != n * nprob {
            return Err(String::from("samples and present must hold nprob * n entries"));
        }
        let mut out = vec![blst_fr::default(); n * nprob];
        match unsafe { kzgamd_poly_recover(self.ctx, out.as_mut_ptr(), samples.as_ptr(), present.as_ptr(), n, nprob, coeffs as c_int) } {
            0 => Ok(out),
            1 => Err(String::from("Samples must have a length that is a power of two")),
            2 => Err(String::from("Impossible to recover, too many shards are missing")),
            3 => Err(String::from(POLY_TOO_WIDE)),
            e => Err(format!("GPU recover failed: {e}")),
        }
    }

    /// (roots a wave of the leaf kernel takes, the longest list for which form 0 takes the direct form)
    pub fn zero_info(&self) -> (usize, usize) {
        let (mut a, mut b) = (0usize, 0usize);
        unsafe { kzgamd_poly_zero_info(self.ctx, &mut a, &mut b) };
        (a, b)
    }

    /// The levels the tree form runs for `count` roots: (polynomials entering, coefficients each, transform length).  Host-only.
    pub fn zero_plan(count: usize) -> Vec<(usize, usize, usize)> {
        let mut lv = [0usize; 96];
        let k = unsafe { kzgamd_poly_zero_plan(count, lv.as_mut_ptr()) };
        (0..k).map(|i| (lv[3 * i], lv[3 * i + 1], lv[3 * i + 2])).collect()
    }

    /// The longest transform a call of this shape enqueues (0: none); op 0 mul by transforms, 1 inverse, 2 div.  Host-only.
    pub fn transform_len(op: i32, la: usize, lb: usize, out_len: usize) -> usize {
        unsafe { kzgamd_poly_transform_len(op as c_int, la, lb, out_len) }
    }
}

impl Drop for GpuPoly {
    fn drop(&mut self) {
        unsafe { kzgamd_poly_free(self.ctx) }
    }
}

/// Sum of Jacobian points on the host: each rank of a multi-GPU MSM contributes one partial.
pub fn g1_sum(partials: &[blst_p1]) -> blst_p1 {
    let mut out = blst_p1::default();
    unsafe { kzgamd_g1_sum(&mut out, partials.as_ptr(), partials.len()) };
    out
}

/// The c-kzg-4844 surface of libkzg_mi355x.so under its exact names (include/kzg_mi355x.h, B3): the same
/// signatures the blst crate exports with `#[no_mangle]` (blst/src/eip_4844.rs:160-530, blst/src/eip_7594.rs:35-44,
/// kzg/src/eth/c_bindings.rs:202-372), so that the binding test-suite (kzg-bench/src/tests/c_bindings.rs) and any
/// consumer of the reference's C API can be pointed at the GPU library.  A process must not also link the blst crate
/// with its `c_bindings` feature (duplicate symbols): use libkzg_mi355x_prefixed.so for that.
pub mod ckzg {
    use kzg::eth::c_bindings::{Blob, Bytes32, Bytes48, CKZGSettings, CKzgRet, Cell, KZGCommitment, KZGProof};
    use libc::FILE;

    extern "C" {
        pub fn load_trusted_setup(out: *mut CKZGSettings, g1_monomial_bytes: *const u8, num_g1_monomial_bytes: u64,
                                  g1_lagrange_bytes: *const u8, num_g1_lagrange_bytes: u64, g2_monomial_bytes: *const u8,
                                  num_g2_monomial_bytes: u64, precompute: u64) -> CKzgRet;
        pub fn load_trusted_setup_file(out: *mut CKZGSettings, in_: *mut FILE) -> CKzgRet;
        pub fn free_trusted_setup(s: *mut CKZGSettings);
        pub fn blob_to_kzg_commitment(out: *mut KZGCommitment, blob: *const Blob, s: &CKZGSettings) -> CKzgRet;
        pub fn compute_kzg_proof(proof_out: *mut KZGProof, y_out: *mut Bytes32, blob: *const Blob, z_bytes: *const Bytes32,
                                 s: &CKZGSettings) -> CKzgRet;
        pub fn compute_blob_kzg_proof(out: *mut KZGProof, blob: *const Blob, commitment_bytes: *const Bytes48,
                                      s: &CKZGSettings) -> CKzgRet;
        pub fn verify_kzg_proof(ok: *mut bool, commitment_bytes: *const Bytes48, z_bytes: *const Bytes32, y_bytes: *const Bytes32,
                                proof_bytes: *const Bytes48, s: &CKZGSettings) -> CKzgRet;
        pub fn verify_blob_kzg_proof(ok: *mut bool, blob: *const Blob, commitment_bytes: *const Bytes48,
                                     proof_bytes: *const Bytes48, s: &CKZGSettings) -> CKzgRet;
        pub fn verify_blob_kzg_proof_batch(ok: *mut bool, blobs: *const Blob, commitments_bytes: *const Bytes48,
                                           proofs_bytes: *const Bytes48, n: usize, s: &CKZGSettings) -> CKzgRet;
        pub fn compute_cells_and_kzg_proofs(cells: *mut Cell, proofs: *mut KZGProof, blob: *const Blob, s: &CKZGSettings) -> CKzgRet;
        pub fn recover_cells_and_kzg_proofs(recovered_cells: *mut Cell, recovered_proofs: *mut KZGProof, cell_indices: *const u64,
                                            cells: *const Cell, num_cells: u64, s: &CKZGSettings) -> CKzgRet;
        pub fn kzgamd_recover_cells_and_kzg_proofs_batch(recovered_cells: *mut Cell, recovered_proofs: *mut KZGProof,
                                                         cell_indices: *const u64, cells: *const Cell, num_cells: *const u64,
                                                         n: usize, s: &CKZGSettings) -> CKzgRet;
        pub fn verify_cell_kzg_proof_batch(ok: *mut bool, commitments_bytes: *const Bytes48, cell_indices: *const u64,
                                           cells: *const Cell, proofs_bytes: *const Bytes48, num_cells: u64, s: &CKZGSettings) -> CKzgRet;
        /// `nbatch` cell-proof batches (data-column sidecars) under one pairing; batch b owns the next `num_cells[b]`
        /// entries of the four arrays.  `ok_each` and `rho` may be null (`rho`: derived from the batches' challenges).
        pub fn kzgamd_verify_cell_kzg_proof_batch_many(ok: *mut bool, ok_each: *mut bool, commitments_bytes: *const Bytes48,
                                                       cell_indices: *const u64, cells: *const Cell, proofs_bytes: *const Bytes48,
                                                       num_cells: *const u64, nbatch: usize, rho: *const blst::blst_fr,
                                                       s: &CKZGSettings) -> CKzgRet;
        pub fn kzgamd_verify_cell_kzg_proof_batch_many_g1(out: *mut blst::blst_p1, commitments_bytes: *const Bytes48,
                                                          cell_indices: *const u64, cells: *const Cell,
                                                          proofs_bytes: *const Bytes48, num_cells: *const u64, nbatch: usize,
                                                          rho: *const blst::blst_fr, s: &CKZGSettings) -> CKzgRet;
        pub fn kzgamd_vcells_info(slice_cells: *mut usize) -> core::ffi::c_int;
        // batched pairing checks on the GPU, one wave per check: ok[i] = e(a1[i], *a2) == e(b1[i], *b2)
        pub fn kzgamd_pairings_verify_batch(ok: *mut bool, a1: *const blst::blst_p1, a2: *const blst::blst_p2,
                                            b1: *const blst::blst_p1, b2: *const blst::blst_p2, count: usize) -> core::ffi::c_int;
        pub fn kzgamd_pairing_info(slice_checks: *mut usize) -> core::ffi::c_int;
        // batched and multi-GPU forms (new API, include/kzg_mi355x.h): contiguous slabs of the batch per settings object
        pub fn kzgamd_blob_to_kzg_commitment_batch(out: *mut KZGCommitment, blobs: *const Blob, n: usize, s: &CKZGSettings) -> CKzgRet;
        pub fn kzgamd_compute_blob_kzg_proof_batch(out: *mut KZGProof, blobs: *const Blob, commitments: *const Bytes48, n: usize,
                                                   s: &CKZGSettings) -> CKzgRet;
        pub fn kzgamd_load_trusted_setup_file_multi(out: *mut CKZGSettings, devices: *const core::ffi::c_int, ndev: usize,
                                                    in_: *mut FILE) -> CKzgRet;
        pub fn kzgamd_free_trusted_setup_multi(s: *mut CKZGSettings, ndev: usize);
        pub fn kzgamd_blob_to_kzg_commitment_batch_multi(out: *mut KZGCommitment, blobs: *const Blob, n: usize,
                                                         s: *const *const CKZGSettings, ndev: usize) -> CKzgRet;
        pub fn kzgamd_compute_blob_kzg_proof_batch_multi(out: *mut KZGProof, blobs: *const Blob, commitments: *const Bytes48,
                                                         n: usize, s: *const *const CKZGSettings, ndev: usize) -> CKzgRet;
        pub fn kzgamd_verify_blob_kzg_proof_batch_multi(ok: *mut bool, blobs: *const Blob, commitments: *const Bytes48,
                                                        proofs: *const Bytes48, n: usize, s: *const *const CKZGSettings,
                                                        ndev: usize) -> CKzgRet;
        pub fn kzgamd_pin_host_buffer(p: *mut core::ffi::c_void, bytes: usize) -> core::ffi::c_int;
        pub fn kzgamd_unpin_host_buffer(p: *mut core::ffi::c_void) -> core::ffi::c_int;
        pub fn kzgamd_device_count() -> core::ffi::c_int;
        /// the slab [lo, hi) the `_multi` entry points give settings object `k` of `parts` for a batch of `n`
        pub fn kzgamd_shard_range(n: usize, parts: usize, k: usize, lo: *mut usize, hi: *mut usize) -> core::ffi::c_int;
    }
}
