//! kzg-bench/src/tests/zero_poly.rs for the MI355X backend (blst/tests/zero_poly.rs): the products run in
//! `zeropoly.hip`; `zero_poly_known` holds them to the reference's precomputed elements.
#[macro_use]
mod common;

use kzg_bench::tests::zero_poly::*;
use rust_kzg_mi355x::{FsFr, FsPoly, MiFFTSettings};

case!(test_reduce_partials_, test_reduce_partials::<FsFr, MiFFTSettings, FsPoly>());
case!(reduce_partials_random_, reduce_partials_random::<FsFr, MiFFTSettings, FsPoly>());
case!(check_test_data_, check_test_data::<FsFr, MiFFTSettings, FsPoly>());
case!(zero_poly_known_, zero_poly_known::<FsFr, MiFFTSettings, FsPoly>());
case!(zero_poly_random_, zero_poly_random::<FsFr, MiFFTSettings, FsPoly>());
case!(zero_poly_all_but_one_, zero_poly_all_but_one::<FsFr, MiFFTSettings, FsPoly>());
case!(zero_poly_252_, zero_poly_252::<FsFr, MiFFTSettings, FsPoly>());
