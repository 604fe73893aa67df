//! `FK20SingleSettings` / `FK20MultiSettings` for the MI355X backend: the reference's
//! blst/src/types/fk20_single_settings.rs and fk20_multi_settings.rs with the whole call on the GPU
//! (`kzgamd_fk20_new` / `kzgamd_fk20_da`, rust-kzg_amd/csrc/fk20.hip): Toeplitz gather, Fr transforms, the pointwise
//! products (a scalar multiplication per product, or a wide fixed-base table when it fits the budget), both G1
//! transforms.  Error strings are the reference's.  Like the rest of this crate: source only, never compiled in the
//! build image (no cargo there); the C side behind it is built and tested (tests/test_fk20_gpu.py).
extern crate alloc;

use alloc::string::String;
use alloc::sync::Arc;
use alloc::vec::Vec;

use blst::{blst_fr, blst_p1};
use kzg::{FK20MultiSettings, FK20SingleSettings, Poly};
use rust_kzg_blst::types::fp::FsFp;
use rust_kzg_blst::types::fr::FsFr;
use rust_kzg_blst::types::g2::FsG2;
use rust_kzg_blst::types::poly::FsPoly;
use rust_kzg_mi355x_sys::GpuFk20;

use crate::fft_settings::MiFFTSettings;
use crate::g1::{MiG1, MiG1Affine, MiG1ProjAddAffine};
use crate::kzg_settings::MiKZGSettings;

/// One device handle for a (n2, chunk_len); `None` only for `Default::default()` (a host placeholder, as elsewhere in
/// this crate: using it is an error, never a CPU fallback).
#[derive(Clone, Default)]
pub struct MiFK20MultiSettings {
    pub kzg_settings: MiKZGSettings,
    pub chunk_len: usize,
    pub gpu: Option<Arc<GpuFk20>>,
}

/// The single form is the multi form with chunk_len = 1 (the same Toeplitz rows, one file).
#[derive(Clone, Default)]
pub struct MiFK20SingleSettings(pub MiFK20MultiSettings);

fn create(ks: &MiKZGSettings, n2: usize, chunk_len: usize) -> Result<MiFK20MultiSettings, String> {
    let ntt = ks.fs.gpu.clone().ok_or_else(|| String::from("MiFFTSettings::default() has no device context; use new(scale)"))?;
    let mono = unsafe { core::slice::from_raw_parts(ks.g1_values_monomial.as_ptr() as *const blst_p1, ks.g1_values_monomial.len()) };
    let gpu = GpuFk20::new(ntt, mono, n2, chunk_len, None)?;
    Ok(MiFK20MultiSettings { kzg_settings: ks.clone(), chunk_len, gpu: Some(Arc::new(gpu)) })
}

fn prove(s: &MiFK20MultiSettings, p: &FsPoly, optimized: bool) -> Result<Vec<MiG1>, String> {
    let n2 = p.len() * 2;
    if n2 > s.kzg_settings.fs.inner.max_width {
        return Err(String::from("n2 must be less than or equal to kzg settings max width"));
    } else if !n2.is_power_of_two() {
        return Err(String::from("n2 must be a power of two"));
    }
    let gpu = s.gpu.as_deref().ok_or_else(|| String::from("FK20 settings built with default() have no device handle"))?;
    let coeffs = unsafe { core::slice::from_raw_parts(p.coeffs.as_ptr() as *const blst_fr, p.coeffs.len()) };
    Ok(gpu.data_availability(coeffs, 1, optimized)?.into_iter().map(MiG1::from_blst).collect())
}

impl FK20MultiSettings<FsFr, MiG1, FsG2, MiFFTSettings, FsPoly, MiKZGSettings, FsFp, MiG1Affine, MiG1ProjAddAffine>
    for MiFK20MultiSettings
{
    fn new(ks: &MiKZGSettings, n2: usize, chunk_len: usize) -> Result<Self, String> {
        create(ks, n2, chunk_len)
    }
    fn data_availability(&self, p: &FsPoly) -> Result<Vec<MiG1>, String> {
        prove(self, p, false)
    }
    fn data_availability_optimized(&self, p: &FsPoly) -> Result<Vec<MiG1>, String> {
        prove(self, p, true)
    }
}

impl FK20SingleSettings<FsFr, MiG1, FsG2, MiFFTSettings, FsPoly, MiKZGSettings, FsFp, MiG1Affine, MiG1ProjAddAffine>
    for MiFK20SingleSettings
{
    fn new(ks: &MiKZGSettings, n2: usize) -> Result<Self, String> {
        Ok(Self(create(ks, n2, 1)?))
    }
    fn data_availability(&self, p: &FsPoly) -> Result<Vec<MiG1>, String> {
        prove(&self.0, p, false)
    }
    fn data_availability_optimized(&self, p: &FsPoly) -> Result<Vec<MiG1>, String> {
        prove(&self.0, p, true)
    }
}
