//! `PolyRecover` for the MI355X backend: `recover_poly_coeffs_from_samples` and `recover_poly_from_samples`
//! (kzg/src/lib.rs `PolyRecover`; reference shape blst/src/recovery.rs) through `kzgamd_poly_recover`: the zero
//! polynomial of the missing set, the masked product, the shifted division and the transforms all run on the device
//! in one call.  The `Option<Fr>` samples are packed into (values, present): a missing sample's value is never used.
//! The reference fails on a vector without a missing sample (it transforms an empty list); the library returns
//! ifft(samples) / the samples there, and so does this.  The reference's scale tables stop at 65536 coefficients;
//! this call has no such limit.
extern crate alloc;

use alloc::string::String;
use alloc::vec::Vec;

use blst::blst_fr;
use kzg::PolyRecover;
use rust_kzg_blst::types::fr::FsFr;
use rust_kzg_blst::types::poly::FsPoly;

use crate::fft_settings::MiFFTSettings;
use crate::poly::MiPolyExt;

fn pack(samples: &[Option<FsFr>]) -> (Vec<blst_fr>, Vec<u8>) {
    let mut values = Vec::with_capacity(samples.len());
    let mut present = Vec::with_capacity(samples.len());
    for s in samples {
        match s {
            Some(v) => {
                values.push(v.0);
                present.push(1u8);
            }
            None => {
                values.push(blst_fr::default());
                present.push(0u8);
            }
        }
    }
    (values, present)
}

fn recover(samples: &[Option<FsFr>], fs: &MiFFTSettings, coeffs: bool) -> Result<FsPoly, String> {
    let (values, present) = pack(samples);
    let out = fs.poly_handle()?.recover(&values, &present, samples.len(), 1, coeffs)?;
    Ok(FsPoly { coeffs: out.into_iter().map(FsFr).collect() })
}

impl PolyRecover<FsFr, FsPoly, MiFFTSettings> for FsPoly {
    /// recovery.rs:62-172
    fn recover_poly_coeffs_from_samples(samples: &[Option<FsFr>], fs: &MiFFTSettings) -> Result<Self, String> {
        recover(samples, fs, true)
    }

    /// recovery.rs:174-194
    fn recover_poly_from_samples(samples: &[Option<FsFr>], fs: &MiFFTSettings) -> Result<Self, String> {
        recover(samples, fs, false)
    }
}
