//! kzg-bench/src/tests/recover.rs for the MI355X backend (blst/tests/recovery.rs): the whole recovery runs in
//! `zeropoly.hip`, one `kzgamd_poly_recover` call per vector.
#[macro_use]
mod common;

use kzg_bench::tests::recover::*;
use rust_kzg_mi355x::{FsFr, FsPoly, MiFFTSettings};

case!(recover_simple_, recover_simple::<FsFr, MiFFTSettings, FsPoly, FsPoly>());
case!(recover_random_, recover_random::<FsFr, MiFFTSettings, FsPoly, FsPoly>());
case!(more_than_half_missing_, more_than_half_missing::<FsFr, MiFFTSettings, FsPoly, FsPoly>());
