//! kzg-bench/src/tests/fk20_proofs.rs for the MI355X backend (blst/tests/fk20_proofs.rs): the whole data_availability
//! call runs in `fk20.hip`; the proofs are verified by the reference's own pairing checks.
#[macro_use]
mod common;

use kzg_bench::tests::fk20_proofs::*;
use rust_kzg_mi355x::backend::generate_trusted_setup;
use rust_kzg_mi355x::fk20::{MiFK20MultiSettings, MiFK20SingleSettings};
use rust_kzg_mi355x::MiBackend;

case!(single, fk_single::<MiBackend, MiFK20SingleSettings>(&generate_trusted_setup));
case!(single_strided, fk_single_strided::<MiBackend, MiFK20SingleSettings>(&generate_trusted_setup));
case!(multi_settings, fk_multi_settings::<MiBackend, MiFK20MultiSettings>(&generate_trusted_setup));
case!(multi_chunk_len_1_512, fk_multi_chunk_len_1_512::<MiBackend, MiFK20MultiSettings>(&generate_trusted_setup));
case!(multi_chunk_len_16_512, fk_multi_chunk_len_16_512::<MiBackend, MiFK20MultiSettings>(&generate_trusted_setup));
case!(multi_chunk_len_16_16, fk_multi_chunk_len_16_16::<MiBackend, MiFK20MultiSettings>(&generate_trusted_setup));
