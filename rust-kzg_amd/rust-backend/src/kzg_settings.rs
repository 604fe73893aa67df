//! KZG settings for the MI355X backend.
//! Reference shape: blst/src/types/kzg_settings.rs:26-260 (`FsKZGSettings` and its `KZGSettings` impl); the
//! `sppark` arm of `new` (:109-123) is the model for the device table.
extern crate alloc;

use alloc::string::{String, ToString};
use alloc::sync::Arc;
use alloc::vec::Vec;

use blst::{blst_fr, blst_p1, blst_p1_affine, blst_p2};
use kzg::{FFTSettings, G1Affine, KZGSettings, FFTG1, G1};
use rust_kzg_blst::types::fp::FsFp;
use rust_kzg_blst::types::fr::FsFr;
use rust_kzg_blst::types::g1::FsG1;
use rust_kzg_blst::types::g2::FsG2;
use rust_kzg_blst::types::poly::FsPoly;
use rust_kzg_mi355x_sys as sys;
use rust_kzg_mi355x_sys::GpuKzg;

use crate::fft_settings::MiFFTSettings;
use crate::g1::{MiG1, MiG1Affine, MiG1ProjAddAffine, MiPrecomputation};

#[derive(Debug, Clone, Default)]
pub struct MiKZGSettings {
    pub fs: MiFFTSettings,
    pub g1_values_monomial: Vec<MiG1>,
    pub g1_values_lagrange_brp: Vec<MiG1>,
    pub g2_values_monomial: Vec<FsG2>,
    /// device-resident fixed-base tables behind ONE handle: over `g1_values_lagrange_brp` (`prepare_msm`, what
    /// `g1_lincomb` multiplies by) and over the rows of `x_ext_fft_columns` (`kzgamd_msm_attach_matrix`, what
    /// `g1_lincomb_batch` multiplies by) — the reference's `precompute(points, matrix)`
    pub precomputation: Option<Arc<MiPrecomputation>>,
    pub x_ext_fft_columns: Vec<Vec<MiG1>>,
    pub cell_size: usize,
    /// whether the FK20 matrix table was attached; `false` = it did not fit its budget (or the device refused) and
    /// `g1_lincomb_batch` runs row by row — correct, two orders of magnitude slower; callers that care can look
    pub matrix_table_attached: bool,
    /// the polynomial-level calls (`commit_to_poly`, `compute_proof_*`, `check_proof_*`) on the GPU: `kzgamd_kzg_new` over
    /// `g1_values_monomial` / `g2_values_monomial` and the NTT handle of `fs`.  `None` only for `Default::default()` (a
    /// host placeholder, as elsewhere in this crate: using it is an error, never a CPU fallback)
    pub poly_kzg: Option<Arc<GpuKzg>>,
}

/// HBM the fixed-base table over `g1_values_monomial` of the polynomial-level handle may take (see below: several
/// settings objects live side by side in the rust-kzg suites).
pub const MONOMIAL_TABLE_BUDGET_BYTES: u64 = 8 << 30;

/// HBM each of the two fixed-base tables of ONE settings object may take.  The library's default (160 GB per table,
/// capped by what is free) is right for a process that owns a GPU and one settings object; the rust-kzg test and bench
/// suites create several `KZGSettings` side by side (and in parallel), and two tables at the default would leave a
/// second object with tiny tables or none.  24 GB buys window c = 13 (20 additions per scalar: 80 % of the default
/// table's commitments/s, DESIGN.md §6 "throughput per table budget"); 16 GB holds the 128 x 64 FK20 matrix at c = 13.
/// [`MiKZGSettings::set_table_budgets`] rebuilds the tables with other values (0 = the library's default).
pub const LAGRANGE_TABLE_BUDGET_BYTES: u64 = 24 << 30;
pub const MATRIX_TABLE_BUDGET_BYTES: u64 = 16 << 30;

fn prepare(points: &[MiG1], matrix: &[Vec<MiG1>], lagrange_budget: u64, matrix_budget: u64) -> (Option<Arc<MiPrecomputation>>, bool) {
    let mut affines: Vec<MiG1Affine> = alloc::vec![MiG1Affine::default(); points.len()];
    MiG1Affine::into_affines_loc(&mut affines, points);
    let raw = unsafe { core::slice::from_raw_parts(affines.as_ptr() as *const blst_p1_affine, affines.len()) };
    let mut cfg = sys::KzgAmdConfig::default();
    cfg.table_budget_bytes = lagrange_budget;
    let handle = sys::prepare_raw_with(raw, &cfg);
    if handle.is_null() {
        return (None, false);
    }
    let mut attached = false;
    // the matrix rows, flattened row-major (every row has the same length: cell_size)
    let rows = matrix.len();
    let cols = matrix.first().map_or(0, |r| r.len());
    if rows > 0 && cols > 0 && matrix.iter().all(|r| r.len() == cols) {
        let flat: Vec<MiG1> = matrix.iter().flat_map(|r| r.iter().copied()).collect();
        let mut flat_aff: Vec<MiG1Affine> = alloc::vec![MiG1Affine::default(); flat.len()];
        MiG1Affine::into_affines_loc(&mut flat_aff, &flat);
        let flat_raw = unsafe { core::slice::from_raw_parts(flat_aff.as_ptr() as *const blst_p1_affine, flat_aff.len()) };
        // a matrix that does not fit the HBM budget is not an error — g1_lincomb_batch then runs row by row — but it is
        // recorded (MiKZGSettings::matrix_table_attached) and, with KZGAMD_VERBOSE set, said on stderr
        let mut mcfg = sys::KzgAmdConfig::default();
        mcfg.table_budget_bytes = matrix_budget;
        match unsafe { sys::attach_matrix_raw(handle, flat_raw, rows, cols, Some(&mcfg)) } {
            Ok(()) => attached = true,
            Err(_e) => {
                #[cfg(feature = "std")]
                if std::env::var_os("KZGAMD_VERBOSE").is_some() {
                    eprintln!("rust-kzg-mi355x: FK20 matrix table not attached ({} x {}, budget {} bytes): {}", rows, cols, matrix_budget, _e);
                }
            }
        }
    }
    (Some(Arc::new(MiPrecomputation::from_ptr(handle))), attached)
}

// FsG1 is a one-field tuple struct over blst_p1 (`pub struct FsG1(pub blst_p1)`, what `MiG1::from_blst` builds and
// `.0 .0` reads): the view below is only sound while the two have the same layout, so that is checked at compile time
const _: () = assert!(core::mem::size_of::<FsG1>() == core::mem::size_of::<blst_p1>()
    && core::mem::align_of::<FsG1>() == core::mem::align_of::<blst_p1>());

/// `&[MiG1]` as the `blst_p1` array the C ABI takes: MiG1 -> FsG1 by `MiG1::slice_as_fs` (repr(transparent)), FsG1 ->
/// blst_p1 by the layout asserted above
fn p1_slice(v: &[MiG1]) -> &[blst_p1] {
    let fs: &[FsG1] = MiG1::slice_as_fs(v);
    unsafe { core::slice::from_raw_parts(fs.as_ptr() as *const blst_p1, fs.len()) }
}

fn fr_slice(v: &[FsFr]) -> &[blst_fr] {
    unsafe { core::slice::from_raw_parts(v.as_ptr() as *const blst_fr, v.len()) }
}

impl MiKZGSettings {
    fn device(&self) -> Result<&GpuKzg, String> {
        self.poly_kzg.as_deref().ok_or_else(|| String::from("MiKZGSettings::default() has no device handle; use new()"))
    }

    /// `compute_proof_single` / `compute_proof_multi`: the batched call (`kzgamd_kzg_open`) with a batch of one — quotient
    /// and commitment in one device pass, nothing of the polynomial touched on the host
    fn open_one(&self, p: &FsPoly, x: &FsFr, n: usize) -> Result<MiG1, String> {
        let (proofs, _) = self.device()?.open(fr_slice(&p.coeffs), p.coeffs.len(), 1, fr_slice(core::slice::from_ref(x)), n, false)?;
        Ok(MiG1::from_blst(proofs[0]))
    }

    /// `check_proof_single` / `check_proof_multi`: interpolation, its commitment and the subtraction on the GPU, the
    /// pairing on the host inside the library (`kzgamd_kzg_check`)
    fn check_one(&self, com: &MiG1, proof: &MiG1, x: &FsFr, ys: &[FsFr], n: usize) -> Result<bool, String> {
        let ok = self.device()?.check(core::slice::from_ref(&com.0 .0), core::slice::from_ref(&proof.0 .0), fr_slice(core::slice::from_ref(x)),
                                      fr_slice(ys), n)?;
        Ok(ok[0])
    }

    /// Any number of `check_proof_single` (n = 1) / `check_proof_multi` statements under ONE pairing
    /// (`kzgamd_kzg_check_batch`): tuple t is (`commitments[t]`, `proofs[t]`, `xs[t]`, `ys[t * n..(t + 1) * n]`).  The
    /// tuples are weighted by the powers of a challenge the library hashes from the inputs; the points are tested for
    /// the curve and for G1 on the device.  An addition over the reference's trait, for callers that check many
    /// samples at once: `Ok(true)` exactly when every tuple would pass `check_proof_multi`, up to the soundness of the
    /// random weights.
    pub fn check_proofs_batch(&self, commitments: &[MiG1], proofs: &[MiG1], xs: &[FsFr], ys: &[FsFr], n: usize) -> Result<bool, String> {
        if !n.is_power_of_two() {
            return Err(String::from("n is not a power of two"));
        }
        if commitments.len() != xs.len() || proofs.len() != xs.len() || ys.len() != xs.len() * n {
            return Err(String::from("commitments, proofs, xs and ys must describe the same number of tuples"));
        }
        let (com, prf) = (p1_slice(commitments), p1_slice(proofs));
        let (ok, _) = self.device()?.check_batch(com, prf, fr_slice(xs), fr_slice(ys), n, None, false)?;
        Ok(ok)
    }

    /// Rebuilds the two device tables with other HBM budgets (bytes per table; 0 = the library's default of 160 GB
    /// capped by the free HBM — for a process with ONE settings object on a GPU of its own).  The old tables are
    /// released first if this object is their last owner (otherwise when the last clone that shares them goes away).
    pub fn set_table_budgets(&mut self, lagrange_budget_bytes: u64, matrix_budget_bytes: u64) {
        // free the old tables first (they may hold most of the HBM) — if this object is their last owner
        if let Some(old) = self.precomputation.take() {
            if let Ok(old) = Arc::try_unwrap(old) {
                unsafe { sys::free_raw(old.table) };
            }
        }
        let (pre, attached) = prepare(&self.g1_values_lagrange_brp, &self.x_ext_fft_columns, lagrange_budget_bytes, matrix_budget_bytes);
        self.precomputation = pre;
        self.matrix_table_attached = attached;
    }
}

impl KZGSettings<FsFr, MiG1, FsG2, MiFFTSettings, FsPoly, FsFp, MiG1Affine, MiG1ProjAddAffine> for MiKZGSettings {
    /// blst/src/types/kzg_settings.rs:66-136.  The FK20 columns are computed the reference's way — k2 = 2 * n /
    /// cell_size G1-valued transforms of length k2 per offset — but through `FFTG1::fft_g1`, i.e. on the GPU.
    fn new(
        g1_monomial: &[MiG1],
        g1_lagrange_brp: &[MiG1],
        g2_monomial: &[FsG2],
        fft_settings: &MiFFTSettings,
        cell_size: usize,
    ) -> Result<Self, String> {
        if g1_monomial.len() != g1_lagrange_brp.len() {
            return Err("G1 point length mismatch".to_string());
        }
        let n = g1_monomial.len();
        let k = n / cell_size;
        let k2 = 2 * k;
        let mut x_ext_fft_columns = alloc::vec![alloc::vec![MiG1::default(); cell_size]; k2];
        for offset in 0..cell_size {
            // x = [ s^(n - cell_size - 1 - offset - i * cell_size) ]_{i < k - 1}, identity, zero-padded to k2
            let start = n - cell_size - 1 - offset;
            let mut x_ext = alloc::vec![MiG1::identity(); k2];
            for (i, slot) in x_ext.iter_mut().enumerate().take(k - 1) {
                *slot = g1_monomial[start - i * cell_size];
            }
            if k2 > 2 * n || !k2.is_power_of_two() {
                return Err("Invalid input size".to_string());
            }
            let column = fft_settings.fft_g1(&x_ext, false)?;
            for (row, value) in column.into_iter().enumerate() {
                x_ext_fft_columns[row][offset] = value;
            }
        }
        let (precomputation, matrix_table_attached) =
            prepare(g1_lagrange_brp, &x_ext_fft_columns, LAGRANGE_TABLE_BUDGET_BYTES, MATRIX_TABLE_BUDGET_BYTES);
        let poly_kzg = match fft_settings.gpu.clone() {
            Some(ntt) => {
                let mono = unsafe { core::slice::from_raw_parts(g1_monomial.as_ptr() as *const blst_p1, g1_monomial.len()) };
                let g2 = unsafe { core::slice::from_raw_parts(g2_monomial.as_ptr() as *const blst_p2, g2_monomial.len()) };
                let mut cfg = sys::KzgAmdConfig::default();
                cfg.table_budget_bytes = MONOMIAL_TABLE_BUDGET_BYTES;
                Some(Arc::new(GpuKzg::new(ntt, mono, g2, Some(&cfg))?))
            }
            None => None,
        };
        Ok(Self {
            poly_kzg,
            g1_values_monomial: g1_monomial.to_vec(),
            g1_values_lagrange_brp: g1_lagrange_brp.to_vec(),
            g2_values_monomial: g2_monomial.to_vec(),
            fs: fft_settings.clone(),
            precomputation,
            x_ext_fft_columns,
            cell_size,
            matrix_table_attached,
        })
    }

    fn commit_to_poly(&self, poly: &FsPoly) -> Result<MiG1, String> {
        let out = self.device()?.commit(fr_slice(&poly.coeffs), poly.coeffs.len(), 1)?;
        Ok(MiG1::from_blst(out[0]))
    }

    fn compute_proof_single(&self, p: &FsPoly, x: &FsFr) -> Result<MiG1, String> {
        self.open_one(p, x, 1)
    }

    fn check_proof_single(&self, com: &MiG1, proof: &MiG1, x: &FsFr, y: &FsFr) -> Result<bool, String> {
        self.check_one(com, proof, x, core::slice::from_ref(y), 1)
    }

    fn compute_proof_multi(&self, p: &FsPoly, x0: &FsFr, n: usize) -> Result<MiG1, String> {
        self.open_one(p, x0, n)
    }

    fn check_proof_multi(&self, com: &MiG1, proof: &MiG1, x: &FsFr, ys: &[FsFr], n: usize) -> Result<bool, String> {
        if !n.is_power_of_two() {
            return Err(String::from("n is not a power of two"));
        }
        if ys.len() != n {
            return Err(String::from("A list with power-of-two length expected"));
        }
        self.check_one(com, proof, x, ys, n)
    }

    fn get_roots_of_unity_at(&self, i: usize) -> FsFr {
        self.fs.get_roots_of_unity_at(i)
    }
    fn get_fft_settings(&self) -> &MiFFTSettings {
        &self.fs
    }
    fn get_g1_monomial(&self) -> &[MiG1] {
        &self.g1_values_monomial
    }
    fn get_g1_lagrange_brp(&self) -> &[MiG1] {
        &self.g1_values_lagrange_brp
    }
    fn get_g2_monomial(&self) -> &[FsG2] {
        &self.g2_values_monomial
    }
    fn get_precomputation(&self) -> Option<&MiPrecomputation> {
        self.precomputation.as_ref().map(|v| v.as_ref())
    }
    fn get_x_ext_fft_columns(&self) -> &[Vec<MiG1>] {
        &self.x_ext_fft_columns
    }
    fn get_cell_size(&self) -> usize {
        self.cell_size
    }
}

/// The device table is owned by the last clone of the settings.
impl Drop for MiKZGSettings {
    fn drop(&mut self) {
        if let Some(table) = self.precomputation.take() {
            if let Ok(table) = Arc::try_unwrap(table) {
                unsafe { sys::free_raw(table.table) };
            }
        }
    }
}
