//! Polynomial arithmetic on the GPU for the MI355X backend.  The reference's `Poly` trait takes no settings argument
//! (kzg/src/lib.rs `Poly::mul`, `inverse`, `div`, `eval` work on the polynomial alone), so `MiBackend::Poly` stays
//! `FsPoly`; what has a device context is `MiFFTSettings`, and the GPU calls hang off it: the extension trait below,
//! and `FFTSettingsPoly::poly_mul_fft`, the one polynomial entry point of the reference that is handed settings.
//! Reference shape: blst/src/types/poly.rs (eval :42-62, inverse :86-149, div :151-250, mul :252-405).
//! Every result is a field element with one value, so the GPU calls return the reference's coefficients exactly.
extern crate alloc;

use alloc::string::String;
use alloc::sync::Arc;
use alloc::vec::Vec;

use blst::blst_fr;
use kzg::{FFTSettingsPoly, Poly};
use rust_kzg_blst::types::fr::FsFr;
use rust_kzg_blst::types::poly::FsPoly;
use rust_kzg_mi355x_sys::{GpuPoly, PolyMulForm};

use crate::fft_settings::MiFFTSettings;

#[inline]
fn fr_raw(data: &[FsFr]) -> &[blst_fr] {
    // FsFr is repr(transparent)-like over blst_fr (blst/src/types/fr.rs)
    unsafe { core::slice::from_raw_parts(data.as_ptr() as *const blst_fr, data.len()) }
}

fn to_poly(raw: Vec<blst_fr>) -> FsPoly {
    FsPoly { coeffs: raw.into_iter().map(FsFr).collect() }
}

/// The polynomial calls of `libkzg_mi355x` over a settings object's device context.  A handle (`kzgamd_poly_new`: a
/// stream and workspace that grows with the calls) lives for one call here; callers with many calls keep a `GpuPoly` of
/// their own (`poly_handle`) and batch polynomials of one shape into one call.
pub trait MiPolyExt {
    fn poly_handle(&self) -> Result<GpuPoly, String>;
    /// the first `len` coefficients of a * b (`Poly::mul`)
    fn poly_mul(&self, a: &FsPoly, b: &FsPoly, len: usize) -> Result<FsPoly, String>;
    /// the first `len` coefficients of 1 / b (`Poly::inverse`)
    fn poly_inverse(&self, b: &FsPoly, len: usize) -> Result<FsPoly, String>;
    /// the quotient of a by b (`Poly::div`)
    fn poly_div(&self, a: &FsPoly, b: &FsPoly) -> Result<FsPoly, String>;
    /// p(x) for every x (`Poly::eval`, one call for all points)
    fn poly_eval_many(&self, p: &FsPoly, xs: &[FsFr]) -> Result<Vec<FsFr>, String>;
}

impl MiPolyExt for MiFFTSettings {
    fn poly_handle(&self) -> Result<GpuPoly, String> {
        let ntt = self.gpu.as_ref().ok_or_else(|| String::from("MiFFTSettings::default() has no device context; use new(scale)"))?;
        GpuPoly::new(Arc::clone(ntt), None)
    }

    fn poly_mul(&self, a: &FsPoly, b: &FsPoly, len: usize) -> Result<FsPoly, String> {
        if a.len() == 0 || b.len() == 0 {
            return Ok(FsPoly::new(0)); // mul_direct's empty product (poly.rs:253-255)
        }
        let out = self.poly_handle()?.mul(fr_raw(&a.coeffs), a.len(), fr_raw(&b.coeffs), b.len(), len, 1, PolyMulForm::Auto)?;
        Ok(to_poly(out))
    }

    fn poly_inverse(&self, b: &FsPoly, len: usize) -> Result<FsPoly, String> {
        Ok(to_poly(self.poly_handle()?.inverse(fr_raw(&b.coeffs), b.len(), len, 1)?))
    }

    fn poly_div(&self, a: &FsPoly, b: &FsPoly) -> Result<FsPoly, String> {
        Ok(to_poly(self.poly_handle()?.div(fr_raw(&a.coeffs), a.len(), fr_raw(&b.coeffs), b.len(), 1)?))
    }

    fn poly_eval_many(&self, p: &FsPoly, xs: &[FsFr]) -> Result<Vec<FsFr>, String> {
        let ys = self.poly_handle()?.eval(fr_raw(&p.coeffs), p.len(), 1, fr_raw(xs))?;
        Ok(ys.into_iter().map(FsFr).collect())
    }
}

impl FFTSettingsPoly<FsFr, FsPoly, MiFFTSettings> for MiFFTSettings {
    /// blst/src/types/poly.rs:280-289.  With settings: the transform product on their device context (form 2 of
    /// `kzgamd_poly_mul`; "longer than the available max width" when their scale is too small for the product).
    /// Without: there is no device context to run on, and the reference builds host settings of its own for this
    /// call (`mul_fft`, :340-346) — so does this.
    fn poly_mul_fft(a: &FsPoly, b: &FsPoly, len: usize, fs: Option<&MiFFTSettings>) -> Result<FsPoly, String> {
        match fs {
            Some(fs) => {
                if a.len() == 0 || b.len() == 0 {
                    return Ok(to_poly(alloc::vec![blst_fr::default(); len]));
                }
                let out = fs.poly_handle()?.mul(fr_raw(&a.coeffs), a.len(), fr_raw(&b.coeffs), b.len(), len, 1, PolyMulForm::Transform)?;
                Ok(to_poly(out))
            }
            None => b.mul_fft(a, len),
        }
    }
}
