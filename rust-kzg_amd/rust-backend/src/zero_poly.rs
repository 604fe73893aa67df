//! `ZeroPoly` for the MI355X backend: `do_zero_poly_mul_partial`, `reduce_partials` and `zero_poly_via_multiplication`
//! (kzg/src/lib.rs `ZeroPoly`; reference shape blst/src/zero_poly.rs) over the settings' device context, through
//! `kzgamd_poly_zero_partial`, `kzgamd_poly_reduce_partials` and `kzgamd_poly_zero_poly`.  Every output is a field
//! element with one value (a monic product of linear factors and its transform), so the calls return the reference's
//! elements exactly, whichever route the library takes.
extern crate alloc;

use alloc::string::String;
use alloc::vec::Vec;

use blst::blst_fr;
use kzg::ZeroPoly;
use rust_kzg_blst::types::fr::FsFr;
use rust_kzg_blst::types::poly::FsPoly;
use rust_kzg_mi355x_sys::PolyMulForm;

use crate::fft_settings::MiFFTSettings;
use crate::poly::MiPolyExt;

#[inline]
fn fr_raw(data: &[FsFr]) -> &[blst_fr] {
    // FsFr is repr(transparent)-like over blst_fr (blst/src/types/fr.rs)
    unsafe { core::slice::from_raw_parts(data.as_ptr() as *const blst_fr, data.len()) }
}

fn to_frs(raw: Vec<blst_fr>) -> Vec<FsFr> {
    raw.into_iter().map(FsFr).collect()
}

impl ZeroPoly<FsFr, FsPoly> for MiFFTSettings {
    /// zero_poly.rs:56-89, for any number of indices (the reference's callers stay below 256)
    fn do_zero_poly_mul_partial(&self, idxs: &[usize], stride: usize) -> Result<FsPoly, String> {
        let idxs: Vec<u64> = idxs.iter().map(|&i| i as u64).collect();
        Ok(FsPoly { coeffs: to_frs(self.poly_handle()?.zero_partial(&idxs, stride)?) })
    }

    /// zero_poly.rs:91-153
    fn reduce_partials(&self, domain_size: usize, partials: &[FsPoly]) -> Result<FsPoly, String> {
        let lens: Vec<usize> = partials.iter().map(|p| p.coeffs.len()).collect();
        let mut flat: Vec<FsFr> = Vec::with_capacity(lens.iter().sum());
        for p in partials {
            flat.extend_from_slice(&p.coeffs);
        }
        Ok(FsPoly { coeffs: to_frs(self.poly_handle()?.reduce_partials(domain_size, fr_raw(&flat), &lens)?) })
    }

    /// zero_poly.rs:177-313.  The empty list is the reference's short cut (two empty vectors, :185-189); the library
    /// would return the empty product there.
    fn zero_poly_via_multiplication(&self, domain_size: usize, idxs: &[usize]) -> Result<(Vec<FsFr>, FsPoly), String> {
        if idxs.is_empty() {
            return Ok((Vec::new(), FsPoly { coeffs: Vec::new() }));
        }
        let missing: Vec<u64> = idxs.iter().map(|&i| i as u64).collect();
        let (ze, zp) = self.poly_handle()?.zero_poly(domain_size, &missing, &[0, missing.len()], PolyMulForm::Auto)?;
        Ok((to_frs(ze), FsPoly { coeffs: to_frs(zp) }))
    }
}
