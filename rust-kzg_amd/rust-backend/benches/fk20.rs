//! kzg-bench/src/benches/fk20.rs for the MI355X backend (blst/benches/fk_20.rs): data_availability of the single form
//! (n2 = 2^14) and the multi form (n = 2^14, chunk_len 16) at the reference's scale 14.
use criterion::{criterion_group, criterion_main, Criterion};
use kzg_bench::benches::fk20::{bench_fk_multi_da, bench_fk_single_da};
use rust_kzg_mi355x::backend::generate_trusted_setup;
use rust_kzg_mi355x::fk20::{MiFK20MultiSettings, MiFK20SingleSettings};
use rust_kzg_mi355x::MiBackend;

fn single(c: &mut Criterion) {
    bench_fk_single_da::<MiBackend, MiFK20SingleSettings>(c, &generate_trusted_setup)
}
fn multi(c: &mut Criterion) {
    bench_fk_multi_da::<MiBackend, MiFK20MultiSettings>(c, &generate_trusted_setup)
}

criterion_group! {
    name = benches;
    config = Criterion::default().sample_size(10);
    targets = single, multi
}
criterion_main!(benches);
