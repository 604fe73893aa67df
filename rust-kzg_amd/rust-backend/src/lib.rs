//! `rust-kzg-mi355x`: a rust-kzg backend whose hot trait methods run on an AMD MI355X.
//!
//! Element types are the blst backend's (`FsFr`, `FsFp`, `FsG2`, `FsPoly` are used as they are: nothing on the
//! hot path lives in them); the three types that own a hot method are thin wrappers:
//!
//! | this crate            | wraps                  | routed to the GPU                                             |
//! |-----------------------|------------------------|---------------------------------------------------------------|
//! | [`g1::MiG1`]          | `FsG1`                 | `G1LinComb::g1_lincomb` (-> `mult_pippenger[_prepared]`)       |
//! | [`fft_settings::MiFFTSettings`] | `FsFFTSettings` | `FFTFr::fft_fr`, `FFTG1::fft_g1`, `DASExtension::das_fft_extension` |
//! | [`fk20::MiFK20SingleSettings`], [`fk20::MiFK20MultiSettings`] | — (device handle) | `FK20SingleSettings` / `FK20MultiSettings::data_availability[_optimized]` (-> `kzgamd_fk20_da`) |
//! | [`kzg_settings::MiKZGSettings`] | — (own fields)  | `KZGSettings::new` (builds the device table), `commit_to_poly`, `compute_proof_single` |
//! | [`poly::MiPolyExt`] on `MiFFTSettings` | — (device handle per call) | `FFTSettingsPoly::poly_mul_fft` with settings, `poly_mul` / `poly_inverse` / `poly_div` / `poly_eval_many` (-> `kzgamd_poly_*`) |
//! | [`zero_poly`] on `MiFFTSettings`, [`recover`] on `FsPoly` | — (device handle per call) | `ZeroPoly::do_zero_poly_mul_partial` / `reduce_partials` / `zero_poly_via_multiplication`, `PolyRecover::recover_poly[_coeffs]_from_samples` (-> `kzgamd_poly_zero_*`, `kzgamd_poly_recover`) |
//!
//! Mirrors blst/src/types/{g1,fft_settings,kzg_settings}.rs method for method; every other method delegates to
//! the wrapped blst type.  Not compiled in the build image: see Cargo.toml.
#![cfg_attr(not(feature = "std"), no_std)]
extern crate alloc;

pub mod backend;
pub mod fft_settings;
pub mod fk20;
pub mod g1;
pub mod kzg_settings;
pub mod poly;
pub mod recover;
pub mod zero_poly;

pub use backend::MiBackend;
pub use fft_settings::MiFFTSettings;
pub use fk20::{MiFK20MultiSettings, MiFK20SingleSettings};
pub use g1::MiG1;
pub use kzg_settings::MiKZGSettings;
pub use poly::MiPolyExt;
pub use rust_kzg_blst::types::{fp::FsFp, fr::FsFr, g2::FsG2, poly::FsPoly};
