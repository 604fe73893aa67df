/*
 * kzg_mi355x — C ABI of the MI355X-native KZG hot path (libkzg_mi355x.so).
 *
 * Plain pointers and sizes only.  Every entry point names the reference interface it
 * replaces (grandinetech/rust-kzg @ 2025-12-12, paths relative to the repo root).
 * Field elements / points use blst's in-memory layout (kzg/src/eth/c_bindings.rs:429-474):
 * little-endian u64 limbs in Montgomery form.
 *
 * All functions need a gfx950 device; without one they fail (non-zero code / NULL handle)
 * — there is no CPU fallback in this library.
 */
#ifndef KZG_MI355X_H
#define KZG_MI355X_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

/* libkzg_mi355x_prefixed.so (python rust-kzg_amd/build.py --prefixed): the same library with every c-kzg-4844 name
 * exported as kzgamd_ckzg_<name>, for a process that also links the reference's own C bindings (e.g. to compare the
 * two backends in one test binary).  Define
 * KZG_MI355X_PREFIXED before including this header and keep writing the plain names. */
#ifdef KZG_MI355X_PREFIXED
#define load_trusted_setup kzgamd_ckzg_load_trusted_setup
#define load_trusted_setup_file kzgamd_ckzg_load_trusted_setup_file
#define free_trusted_setup kzgamd_ckzg_free_trusted_setup
#define blob_to_kzg_commitment kzgamd_ckzg_blob_to_kzg_commitment
#define compute_kzg_proof kzgamd_ckzg_compute_kzg_proof
#define compute_blob_kzg_proof kzgamd_ckzg_compute_blob_kzg_proof
#define verify_kzg_proof kzgamd_ckzg_verify_kzg_proof
#define verify_blob_kzg_proof kzgamd_ckzg_verify_blob_kzg_proof
#define verify_blob_kzg_proof_batch kzgamd_ckzg_verify_blob_kzg_proof_batch
#define compute_challenge kzgamd_ckzg_compute_challenge
#define bytes_to_kzg_commitment kzgamd_ckzg_bytes_to_kzg_commitment
#define bytes_from_bls_field kzgamd_ckzg_bytes_from_bls_field
#define compute_cells_and_kzg_proofs kzgamd_ckzg_compute_cells_and_kzg_proofs
#define recover_cells_and_kzg_proofs kzgamd_ckzg_recover_cells_and_kzg_proofs
#define verify_cell_kzg_proof_batch kzgamd_ckzg_verify_cell_kzg_proof_batch
#define compute_verify_cell_kzg_proof_batch_challenge kzgamd_ckzg_compute_verify_cell_kzg_proof_batch_challenge
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } blst_fr;
typedef struct { uint64_t l[6]; } blst_fp;
typedef struct { blst_fp x, y; } blst_p1_affine;     /* infinity = all-zero (blst/src/types/g1.rs:303-316) */
typedef struct { blst_fp x, y, z; } blst_p1;          /* Jacobian; infinity = Z == 0 */
typedef struct { blst_fp fp[2]; } blst_fp2;
typedef struct { blst_fp2 x, y, z; } blst_p2;          /* Jacobian over Fp2; infinity = Z == 0 */

/* sppark's error struct, returned by value (arkworks3-sppark-wlc/sppark/util/rusterror.h:15-27):
 * code 0 = ok; message is malloc'ed (caller frees) or NULL */
typedef struct { int code; char *message; } RustError;

/* ------------------------------------------------------------------------------------------
 * Configuration of a handle (new API; the reference's handles take none — its sppark context sizes itself).  Every
 * creating entry point has an _ex form that takes one; NULL means the defaults, which is what the plain names pass.
 * Values are read once, when the handle is created.  Set struct_size = sizeof(KzgAmdConfig) (kzgamd_config_init does).
 * ------------------------------------------------------------------------------------------ */
#define KZGAMD_NO_TABLES UINT64_MAX   /* table_budget_bytes: build no wide fixed-base table at all (bucket engine) */
typedef struct {
    uint32_t struct_size;          /* sizeof(KzgAmdConfig) of the caller's header */
    int32_t device;                /* GPU ordinal the handle lives on; -1 = the calling thread's current device */
    uint64_t table_budget_bytes;   /* HBM EACH fixed-base table of the handle may take (a settings object has up to three:
                                    * commitments, cell proofs, FK20 columns; tables after the first are built at first
                                    * use).  0 = default: 160 GB, capped by what is free less 12 GB of working room */
    const char *tuning;            /* NULL, or "key=value;key=value": the measured switches (kzgamd_tuning_keys lists
                                    * them).  An unknown key or a value out of range fails the call */
} KzgAmdConfig;
void kzgamd_config_init(KzgAmdConfig *cfg);   /* struct_size, device = -1, no budget, no tuning */
/* the tuning keys, one per line: "name default lo hi meaning"; returns a static string */
const char *kzgamd_tuning_keys(void);

/* ------------------------------------------------------------------------------------------
 * B1 — GPU MSM plug-in.  Same three symbols `rust-kzg-blst` binds under feature `sppark`
 * (blst-sppark/src/lib.rs:8-62, defined today by blst-sppark/cuda/pippenger.cu:23-38).
 * Scalars are blst_fr IN MONTGOMERY FORM (blst/src/kzg_proofs.rs:47-48); out is Jacobian.
 * Thread-safe: any number of threads may call on one handle (the reference shares it through an Arc between rayon
 * workers, kzg/src/msm/sppark.rs:24-44).  Concurrent mult_pippenger_prepared calls of the same length (up to 2^16
 * scalars) are combined into batched launches (up to three in flight); other calls serialise on an internal mutex.
 * Bases may be ANY points of the curve, as in the reference (FsG1::from_bytes does not test the subgroup,
 * blst/src/types/g1.rs:65-87): the result is the plain sum of k_i P_i.  The engines' endomorphism (GLV) split is an
 * identity of the r-torsion subgroup G1 only, so every handle tests its bases once at creation and runs unsplit if one
 * fails; mult_pippenger, whose handle lives for one call, tests up to 2^15 bases and runs unsplit beyond.
 * ------------------------------------------------------------------------------------------ */
void *prepare_msm(const blst_p1_affine points[], size_t npoints);
RustError mult_pippenger_prepared(void *msm, blst_p1 *out, size_t npoints, const blst_fr scalars[]);
RustError mult_pippenger(blst_p1 *out, const blst_p1_affine points[], size_t npoints, const blst_fr scalars[]);

/* Additions (the reference leaks the handle; batched shape follows the wlc variant's
 * mult_pippenger_faster_inf(ctx,out,npoints,batches,scalars), arkworks3-sppark-wlc/src/lib.rs:24-42):
 * scalars is nbatch x npoints, out is nbatch points. */
void free_msm(void *msm);
void *kzgamd_prepare_msm_ex(const blst_p1_affine points[], size_t npoints, const KzgAmdConfig *cfg);
RustError mult_pippenger_prepared_batch(void *msm, blst_p1 out[], size_t npoints, size_t nbatch,
                                        const blst_fr scalars[]);

/* Matrix handle: `rows` independent base sets of `cols` points each in ONE table (points[r * cols + c]) — what the
 * reference's precomputation holds for g1_lincomb_batch (BgmwTable.batch_points, kzg/src/msm/bgmw.rs:206-304; FK20's
 * 128 columns of 64 points, kzg/src/das.rs:682-686) and multiplies in multiply_batch (bgmw.rs:306-380):
 *   out[m * rows + r] = sum_c scalars[(m * rows + r) * cols + c] * points[r * cols + c],   m < nmat
 * in one launch for all rows (and all nmat scalar matrices: nmat = 1 is G1LinComb::g1_lincomb_batch,
 * kzg/src/lib.rs:156-181).  Scalars in Montgomery form, out Jacobian, as mult_pippenger_prepared.  The handle needs a
 * wide table (NULL when none fits cfg's budget: rows * cols * 2^9 * 13 slots of 128 B at the least); free_msm frees it;
 * thread-safe like every handle. */
void *kzgamd_prepare_msm_matrix(const blst_p1_affine points[], size_t rows, size_t cols, const KzgAmdConfig *cfg);
RustError kzgamd_mult_pippenger_matrix(void *msm, blst_p1 out[], const blst_fr scalars[], size_t nmat);
/* The matrix as a part of an existing handle (any handle of prepare_msm / kzgamd_settings_msm_handle): the reference's
 * PrecomputationTable is ONE object built from (points, matrix) (precompute(), kzg/src/msm/bgmw.rs:206-304) and the sppark
 * flavour of it has room for one pointer (kzg/src/msm/sppark.rs:5-22) — after this call kzgamd_mult_pippenger_matrix on
 * `msm` multiplies by the attached matrix, mult_pippenger_prepared by its own points as before; free_msm frees both.
 * cfg: the matrix table's budget and tuning (its device is the handle's).  A handle takes ONE matrix, once: a second
 * attach fails (code 1) and leaves the first in place, so a matrix call in flight never sees its table freed. */
RustError kzgamd_msm_attach_matrix(void *msm, const blst_p1_affine points[], size_t rows, size_t cols, const KzgAmdConfig *cfg);
/* rows and columns of the matrix a handle holds or has attached; 1 when it has none */
int kzgamd_msm_matrix_shape(void *msm, size_t *rows, size_t *cols);

/* Device-resident form used by the batched blob pipeline and bench.py: d_scalars / d_out are
 * device pointers, work is enqueued on `stream` (a hipStream_t, NULL = default stream) and NOT
 * synchronised.  scalars_mont != 0: blst_fr Montgomery limbs; 0: canonical little-endian 256-bit.
 * A handle keeps one workspace per stream it is used on, for up to eight streams: calls enqueued on the same
 * stream are serialised by stream order, calls on different streams may overlap on the GPU (the low-occupancy
 * tail of one batch under the accumulation of the next).  With more streams than workspaces the library makes a
 * stream wait (on the GPU) for the previous use of the workspace it is handed: still correct, no longer overlapped.
 * The host-buffer entry points above synchronise internally and may be called from any thread. */
RustError kzgamd_msm_prepared_batch_device(void *msm, void *d_out, const void *d_scalars, size_t npoints,
                                           size_t nbatch, int scalars_mont, void *stream);
/* Allocates now the workspace `stream` will use for nbatch MSMs of npoints scalars, so that the enqueue calls that
 * follow never call hipMalloc (which synchronises the device).  Without it the first enqueue on a new stream, or
 * with a larger shape, allocates lazily. */
RustError kzgamd_msm_reserve(void *msm, size_t npoints, size_t nbatch, void *stream);
/* the GPU a handle lives on (-1 for NULL) */
int kzgamd_msm_device(void *msm);
/* introspection for benches/tests: window bits, table rows, buckets of a handle */
int kzgamd_msm_info(void *msm, int *window_bits, int *rows, size_t *nbuckets, size_t *npoints);
/* non-zero if the handle holds the wide fixed-base table (rows x npoints x 2^(window_bits-1) affine multiples,
 * built when it fits the handle's table budget (KzgAmdConfig.table_budget_bytes; default 160 GB, capped by free HBM)) and so runs the gather-and-add
 * path: 1 = rows cover the 255-bit scalar (rows additions per scalar), 2 = GLV form, rows cover a 128-bit half
 * (2 x rows additions per scalar; chosen only when every base passed the r-torsion test at prepare time) */
int kzgamd_msm_uses_wide_table(void *msm);
/* HIP-event timing of the bucket-accumulation kernel (k_accum) and of the whole enqueue, recorded on
 * the launch stream; set(on) resets; get returns the number of enqueues averaged (-1 if none) */
int kzgamd_msm_set_profile(void *msm, int on);
int kzgamd_msm_get_profile(void *msm, float *accum_ms, float *total_ms);
/* Handle over DEVICE-resident bases (blst_p1_affine[npoints] in HBM); prepare != 0 builds the fixed-base
 * rows like prepare_msm, 0 gives the variable-base engine mult_pippenger uses. */
void *kzgamd_msm_create_device(const void *d_points_affine, size_t npoints, int prepare);
void *kzgamd_msm_create_device_ex(const void *d_points_affine, size_t npoints, int prepare, const KzgAmdConfig *cfg);
/* bench/test utility: npoints distinct G1 points h_i*G (h_i from splitmix64(seed,i), 248 bits) written
 * as blst_p1_affine into device memory */
RustError kzgamd_generate_points(void *d_out_affine, size_t npoints, uint64_t seed, void *stream);

/* ------------------------------------------------------------------------------------------
 * B2 — NTT plug-in.  Replaces FFTFr::fft_fr / DASExtension::das_fft_extension for FsFFTSettings
 * (kzg/src/lib.rs:421-431; blst/src/fft_fr.rs:112-165; blst/src/data_availability_sampling.rs:78-100).
 * Natural order in, natural order out, Montgomery blst_fr; inverse scales by n^-1.
 * Return codes mirror the reference's error conditions:
 *   ntt_fr:            0 ok, 1 "longer than the available max width", 2 "power-of-two length expected"
 *   das_fft_extension: 0 ok, 1 empty, 2 not a power of two, 3 longer than max width / 2
 *   fft_g1:            as ntt_fr
 *   negative: device error
 * Thread-safe: a handle may be shared between threads (FFTSettings is shared by reference in the reference); concurrent
 * ntt_fr / das_fft_extension calls of the same kind and length (up to 8192 elements) are combined into batched launches,
 * everything else serialises on the handle's mutex.
 * ------------------------------------------------------------------------------------------ */
void *kzgamd_ntt_new(unsigned scale);           /* FsFFTSettings::new(scale), blst/src/types/fft_settings.rs:30-58 */
void *kzgamd_ntt_new_ex(unsigned scale, const KzgAmdConfig *cfg);
void kzgamd_ntt_free(void *ctx);
int ntt_fr(void *ctx, blst_fr *out, const blst_fr *in, size_t n, int inverse);
int das_fft_extension(void *ctx, blst_fr *odds, const blst_fr *evens, size_t half_n);
/* G1-valued transform: FFTG1::fft_g1 for FsFFTSettings (kzg/src/lib.rs:433-435; blst/src/fft_g1.rs:54-83).
 * Jacobian blst_p1 in and out (any valid representation in; infinity = Z == 0), natural order, inverse
 * scales by n^-1.  Outputs equal the reference's as group elements (the Jacobian representative differs).
 * kzgamd_fft_g1_batch runs nbatch independent transforms of length n (contiguous) in the same launches —
 * the shape of the 64 x size-128 transforms of the FK20 setup (blst/src/types/kzg_settings.rs:84-101). */
int fft_g1(void *ctx, blst_p1 *out, const blst_p1 *in, size_t n, int inverse);
int kzgamd_fft_g1_batch(void *ctx, blst_p1 *out, const blst_p1 *in, size_t n, size_t nbatch, int inverse);
/* device-resident, batched (nbatch independent transforms of length n, contiguous), on `stream` */
int kzgamd_ntt_fr_device(void *ctx, void *d_out, const void *d_in, size_t n, size_t nbatch, int inverse, void *stream);
/* das_fft_extension on device-resident data: nbatch contiguous lists of half_n elements; d_scratch (half_n * nbatch
 * elements) must differ from d_odds and d_evens, which must not alias each other (-3).  Two half-size transforms:
 * the twist by the 2n-th roots and the n^-1 ride in their last-pass multiplications. */
int kzgamd_das_fft_extension_device(void *ctx, void *d_odds, const void *d_evens, void *d_scratch, size_t half_n,
                                    size_t nbatch, void *stream);
/* host copies of the settings arrays (FFTSettings getters, kzg/src/lib.rs:465-481); counts in elements */
int kzgamd_ntt_roots(void *ctx, blst_fr *roots /*W+1*/, blst_fr *reverse_roots /*W+1*/, blst_fr *brp_roots /*W*/);
/* Generic FK20 data-availability proofs for any polynomial length n = n2 / 2 and chunk length:
 * FK20SingleSettings (chunk_len = 1, blst/src/types/fk20_single_settings.rs:38-111) and FK20MultiSettings
 * (blst/src/types/fk20_multi_settings.rs:60-175), npoly polynomials per call.  With k2 = n2 / chunk_len the handle keeps
 * the k2 x chunk_len points fft_g1(x_i)[j] on the GPU, either for a scalar multiplication per product (form 1, always
 * available) or as a wide fixed-base table of k2 base sets (form 2: taken when the table fits cfg->table_budget_bytes —
 * k2 * chunk_len * 2^9 * 13 slots of 128 B at the least; "fk20_table=0" in cfg->tuning: never, "fk20_table=1": required.
 * fk20_table is a key of this entry point alone, read from cfg->tuning only: it is not in kzgamd_tuning_keys() and the
 * other handle types refuse it like any unknown key).  Proofs equal the
 * reference's as group elements.  The setup points must lie in G1 (both forms split scalars with the endomorphism).
 *
 * kzgamd_fk20_new: FK20SingleSettings::new / FK20MultiSettings::new.  `ntt` = kzgamd_ntt_new(scale) with 2^scale >= n2
 * (roots are taken with stride max_width / k2, as fft_g1 does).  The FK20 handle keeps `ntt` by pointer and uses it in
 * every call: free the FK20 handle FIRST, the NTT handle after it.  g1_monomial = [s^i]G, i < num_g1, Jacobian; needs
 * num_g1 >= n2/2 - chunk_len.  *err (may be NULL): 0 ok, 1 n2 > max width, 2 n2 not a power of two, 3 n2 < 2,
 * 4 chunk_len > n2/2, 5 chunk_len not a power of two (or 0), 6 too few setup points — the reference's checks in the
 * reference's order — negative = NULL argument (-1), malformed configuration (-2), fk20_table = 1 without room (-3) or a
 * device error.  Returns NULL on any error.  kzgamd_fk20_free gives every byte of HBM back.
 *
 * kzgamd_fk20_da: npoly polynomials of n = n2/2 Montgomery coefficients each (contiguous) -> npoly x (n2 / chunk_len)
 * proofs, Jacobian.  optimized != 0: data_availability_optimized (natural order); 0: data_availability (bit-reversed per
 * polynomial).  0 ok, 3 n != n2/2, -1 NULL argument, other negatives = device error.  npoly = 0: ok, nothing written.
 * Thread-safe like every handle (calls on one handle take turns; fft_g1 / ntt_fr calls on `ntt` may run beside them).
 *
 * kzgamd_fk20_info: n2, chunk_len and the form in use (1 = direct, 2 = table); any pointer may be NULL. */
void *kzgamd_fk20_new(void *ntt, const blst_p1 *g1_monomial, size_t num_g1, size_t n2, size_t chunk_len,
                      const KzgAmdConfig *cfg, int *err);
void kzgamd_fk20_free(void *fk);
int kzgamd_fk20_da(void *fk, blst_p1 *out, const blst_fr *polys, size_t n, size_t npoly, int optimized);
int kzgamd_fk20_info(void *fk, size_t *n2, size_t *chunk_len, int *form);
/* Generic polynomial KZG, the proving and checking calls of KZGSettings (blst/src/types/kzg_settings.rs:138-277):
 * commit_to_poly, compute_proof_single, compute_proof_multi, check_proof_single, check_proof_multi — for any setup
 * [s^i]G, batched.  Scalars are Montgomery blst_fr, points Jacobian, results equal the reference's as group elements.
 * The quotient of p by X^n - x^n is computed on the GPU (rust-kzg_amd/csrc/kzg.hip: one lane per residue class mod n
 * when the call has lane_form_min such lanes, otherwise a scan over chunks of `chunk` steps — kzgamd_kzg_info gives
 * both); a call makes one upload, one batched MSM and one download (per slice of pairs, when its workspace would take
 * more than a share of the free HBM).
 *
 * kzgamd_kzg_new: `ntt` = kzgamd_ntt_new(scale); the coset of length n is x * <roots[max_width / n]>.  The handle keeps
 * `ntt` by pointer and uses it in every call: free the KZG handle FIRST, the NTT handle after it.  g1_monomial = [s^i]G,
 * i < num_g1, Jacobian, any points of the curve (the bases are tested for G1 at creation like prepare_msm's; cfg gives
 * the table budget and the tuning of the MSM handle over them).  g2_monomial = [s^i]G2, i < num_g2, copied; NULL / 0: a
 * handle that proves but does not check.  *err (may be NULL): 0 ok, 1 num_g1 == 0; negative = NULL argument (-1),
 * malformed configuration (-2) or a device error.  Returns NULL on any error.  kzgamd_kzg_free gives every byte of HBM
 * back.  Thread-safe like every handle (calls on one handle take turns; calls on `ntt` may run beside them).
 *
 * kzgamd_kzg_commit: out[b] = sum_i polys[b * len + i] * g1_monomial[i], b < npoly (commit_to_poly, :138-153).
 * 0 ok, 1 len > num_g1 ("Polynomial is longer than secret g1"), -1 NULL argument, other negatives = device error.
 * len = 0: identities; npoly = 0: ok, nothing written.
 *
 * kzgamd_kzg_open: every (polynomial, x) pair of npoly polynomials of len coefficients and nx points in one call:
 * proofs[b * nx + k] = commitment to q with p_b = q (X^n - x_k^n) + r, deg r < n — compute_proof_single (:155-176) for
 * n = 1, compute_proof_multi (:198-234) for n > 1.  0 ok, 2 len == 0 ("Polynomial must not be empty"), 3 n is zero or
 * not a power of two, 1 len - n > num_g1, 4 ys != NULL and n > max width of `ntt`; negatives as above.  len <= n gives
 * the identity (the reference's zero-length quotient, blst/src/types/poly.rs:167-170, 226-229).  npoly = 0 or nx = 0:
 * ok, nothing written.  ys (may be NULL; an addition over the reference, whose callers evaluate with Poly::eval):
 * ys[(b * nx + k) * n + i] = p_b(x_k w^i), w = roots[max_width / n] — from the remainder, by one batched transform.
 *
 * kzgamd_kzg_check: count tuples (commitment, proof, x, n values) in one call; ok[t] = the pairing equation holds:
 *   n = 1 (check_proof_single, :178-196):  e(com - [y]g1_monomial[0], G2) == e(proof, [s]G2 - [x]G2)
 *   n > 1 (check_proof_multi, :236-277):   e(com - [I(s)]G, G2) == e(proof, [s^n]G2 - [x^n]G2), I = the interpolation
 *         polynomial of the values on the coset: ifft(ys), coefficient i times x^-i.
 * The G1 sides run on the GPU for all tuples together.  Below the handle's tuning key pairing_gpu_min (tuples per
 * call; 0 = never) the G2 sides and one pairing per tuple run on the host (as in the reference); from it on the pairings
 * run on the GPU, one wave per tuple, as e(lhs + [x^n] proof, G2) == e(proof, [s^n]G2) against device line tables kept per
 * handle and n — for the tuples whose commitment and proof are in G1 (tested on the GPU); the others, and every tuple
 * of a call with a point off the curve, take the host loop, so the verdicts are the same for every input.
 * pairing_gpu_min is a key of kzgamd_kzg_new alone, read from cfg->tuning only (-1 ... 1048576; -1, the default, is the
 * measured built-in, 4): it is not in kzgamd_tuning_keys() and the environment does not carry it.  0 ok, 3 n is zero or not a power of two, 4 n > max width, 6 num_g2 <= n (or no G2 setup), 1 n > num_g1,
 * 5 x == 0 in a tuple with n > 1 — the reference feeds inverse(0) into its arithmetic there (:253-261), which has no
 * meaningful result; negatives as above.  count = 0: ok, nothing written.
 *
 * kzgamd_kzg_check_batch: the same count tuples under ONE pairing.  With weights rho_t = r^t (rho_0 = 1), I_t the
 * interpolation polynomial of tuple t as above and A = sum_t rho_t I_t (n coefficients):
 *   L = sum rho_t com_t + sum rho_t x_t^n proof_t - [A(s)]G,   P = sum rho_t proof_t,   *ok = e(L, G2) == e(P, [s^n]G2)
 * — kzgamd_kzg_check's equation with [x_t^n]G2 moved to the G1 side, summed with the weights.  If every tuple is valid
 * the batch passes for every r; if one is not, and every point is in G1, it passes for at most count - 1 values of r.  So
 * the points are tested (on the curve and in G1, on the GPU) and r must not be known before the inputs are:
 *   r == NULL: r = kzgamd_kzg_batch_challenge of the inputs;
 *   r != NULL: used as given, for callers with a transcript of their own (and for tests).  Such an r MUST be fixed
 *     after every input of the call is: an r the prover can anticipate lets errors of different tuples cancel (r = 1 adds
 *     the tuples up unweighted, r = 0 checks tuple 0 alone).
 * Everything but the hash and one pairing against line tables kept per handle and n runs on the GPU: the points to affine
 * form with one inversion per lane and both tests, the weights, A from one batched inverse transform, [A(s)]G, one
 * two-row MSM over the 2 count points.  Codes: kzgamd_kzg_check's, in its order (3, 4, 6, 1, 5), then 7 a commitment
 * or proof is not on the curve or not in G1; -1 NULL argument, other negatives = device error.  On a positive code
 * nothing is written.  count = 0: ok, *ok = true (ok is still required; the input pointers are not looked at).  Point
 * coordinates are taken mod p (a non-canonical limb pattern >= p is the element it reduces to); the identity is Z = 0
 * with all-zero limbs, whatever X and Y hold.  The derived challenge is hashed before the handle's lock is taken, the
 * pairing runs after it is released.  ok_each (may be NULL): when the batch passes every entry is true;
 * when it fails the entries are kzgamd_kzg_check's for the same tuples (count pairings).
 *
 * kzgamd_kzg_check_batch_g1: L and P (out[0], out[1], Jacobian) of the same inputs and the same r, no pairing — for
 * callers that pair themselves, like kzgamd_verify_kzg_proof_batch_g1.  Needs no G2 setup: code 6 does not apply.
 * count = 0: two identities (out is still required).
 *
 * kzgamd_kzg_batch_challenge (host only, no GPU): r = hash_to_bls_field(SHA-256(D)) — the digest as a big-endian
 * integer mod the group order, as compute_challenge reduces its digest — with D = "KZGAMD_CHKBATCH1" (16 bytes) |
 * u64_be(n) | u64_be(count) | the count x 144 commitment bytes | the count x 144 proof bytes | the count x 32 bytes of
 * xs | the count x n x 32 bytes of ys, all AS PASSED: the caller's in-memory bytes, not a canonical encoding (no
 * inversion, and the hash runs on the host while the GPU works).  Two Jacobian forms of one point therefore give two
 * challenges — each as good as the other, but a verifier that must reproduce r has to hash the same bytes.  0 ok, -1
 * NULL argument.
 *
 * kzgamd_kzg_info: the setup sizes, the chunk length of the scan form and the number of lanes (pairs x n) from which
 * the lane form is taken; any pointer may be NULL. */
void *kzgamd_kzg_new(void *ntt, const blst_p1 *g1_monomial, size_t num_g1, const blst_p2 *g2_monomial, size_t num_g2,
                     const KzgAmdConfig *cfg, int *err);
void kzgamd_kzg_free(void *kz);
int kzgamd_kzg_info(void *kz, size_t *num_g1, size_t *num_g2, size_t *chunk, size_t *lane_form_min);
int kzgamd_kzg_commit(void *kz, blst_p1 *out, const blst_fr *polys, size_t len, size_t npoly);
int kzgamd_kzg_open(void *kz, blst_p1 *proofs, blst_fr *ys, const blst_fr *polys, size_t len, size_t npoly,
                    const blst_fr *xs, size_t nx, size_t n);
int kzgamd_kzg_check(void *kz, bool *ok, const blst_p1 *commitments, const blst_p1 *proofs, const blst_fr *xs,
                     const blst_fr *ys, size_t n, size_t count);
int kzgamd_kzg_check_batch(void *kz, bool *ok, bool *ok_each, const blst_p1 *commitments, const blst_p1 *proofs,
                           const blst_fr *xs, const blst_fr *ys, size_t n, size_t count, const blst_fr *r);
int kzgamd_kzg_check_batch_g1(void *kz, blst_p1 out[2], const blst_p1 *commitments, const blst_p1 *proofs,
                              const blst_fr *xs, const blst_fr *ys, size_t n, size_t count, const blst_fr *r);
int kzgamd_kzg_batch_challenge(blst_fr *r_out, const blst_p1 *commitments, const blst_p1 *proofs, const blst_fr *xs,
                               const blst_fr *ys, size_t n, size_t count);
/* Batched polynomial arithmetic, the reference's Poly<Fr> and FFTSettingsPoly (blst/src/types/poly.rs) on the GPU
 * (rust-kzg_amd/csrc/poly.hip).  Conventions of kzgamd_kzg_*: scalars are Montgomery blst_fr in host buffers; batches
 * are contiguous, npoly independent problems of the same shape per call; the handle is thread-safe (calls on one handle
 * take turns; calls on `ntt` may run beside them).  Codes: 0 ok, positive = the reference's error conditions as listed
 * per call, -1 NULL argument (or a form outside 0..2), other negatives = device error.  Every result is a field element
 * with one value — a truncated product, the first coefficients of a power-series inverse, a quotient by a divisor whose
 * highest coefficient is non-zero — so results equal the reference's element for element, whichever route runs.
 *
 * kzgamd_poly_new keeps `ntt` by pointer and uses it in every call: free the poly handle FIRST, the NTT handle after
 * it.  *err (may be NULL): 0 ok, -1 NULL argument, -2 malformed configuration, -(100 + hipError_t) a device error, -4 any
 * other failure (out of host memory).  kzgamd_poly_free
 * gives every byte of HBM back.  kzgamd_poly_info: the max width of `ntt`, the coefficients a lane of eval takes, the
 * multiplications per lane up to which form 0 of mul takes the direct product, the coefficients of an inverse that
 * come from the one-launch recurrence before Newton steps begin; any pointer may be NULL. */
void *kzgamd_poly_new(void *ntt, const KzgAmdConfig *cfg, int *err);
void kzgamd_poly_free(void *ph);
int kzgamd_poly_info(void *ph, size_t *max_width, size_t *eval_chunk, size_t *mul_direct_max, size_t *inv_direct_max);
/* ys[b * nx + k] = p_b(x_k) (Poly::eval, poly.rs:42-62).  len = 0: zeros.  x = 0 gives coefficient 0.  npoly = 0 or
 * nx = 0: ok, nothing written. */
int kzgamd_poly_eval(void *ph, blst_fr *ys, const blst_fr *polys, size_t len, size_t npoly, const blst_fr *xs, size_t nx);
/* out[b * len + i] = in[b * len + i] * 5^-(i+1) (inverse = 0: Poly::scale, poly.rs:64-73) or * 5^(i+1) (inverse = 1:
 * unscale, :75-83).  NOTE the exponent i + 1, not i: the reference multiplies before it uses the power.  out may be in. */
int kzgamd_poly_scale(void *ph, blst_fr *out, const blst_fr *in, size_t len, size_t npoly, int inverse);
/* out[b * out_len + i] = coefficient i of a_b * b_b, zero beyond la + lb - 2 (mul_direct :252-277, mul_fft :340-396,
 * mul :398-405).  form 0: chosen by shape, 1: direct (a lane per output coefficient), 2: by transforms (a product of
 * two constants runs none).  All forms give the same elements.  la = 0 or lb = 0: out_len zeros (the reference returns
 * an empty polynomial there).  out_len = 0 or npoly = 0: ok, nothing written.  4: the transform form needs a transform
 * longer than the handle's max width (nothing written). */
int kzgamd_poly_mul(void *ph, blst_fr *out, const blst_fr *a, size_t la, const blst_fr *b, size_t lb, size_t out_len,
                    size_t npoly, int form);
/* out[b * out_len + i] = coefficient i of 1 / b_b as a power series (Poly::inverse, :86-149).  1: out_len == 0,
 * 2: lb == 0, 3: a polynomial of the batch has b[0] == 0 (outputs unspecified), 4: as above. */
int kzgamd_poly_inverse(void *ph, blst_fr *out, const blst_fr *b, size_t lb, size_t out_len, size_t npoly);
/* q[b * (la - lb + 1) + i] = coefficient i of the quotient of a_b by b_b (div :151-158, long_div :160-214, fast_div
 * :216-250: one result whichever the reference would take).  1: lb == 0 ("Can't divide by zero"), 2: a divisor's
 * highest coefficient is zero (outputs unspecified), 4: as above.  la < lb: ok, nothing written (the reference's
 * zero-length quotient). */
int kzgamd_poly_div(void *ph, blst_fr *q, const blst_fr *a, size_t la, const blst_fr *b, size_t lb, size_t npoly);
/* host-only, no GPU: the longest transform a call of this shape enqueues in this build (0: none).  op 0 mul (form 2),
 * 1 inverse (la ignored), 2 div (out_len ignored).  A call succeeds exactly when the handle's max width is at least
 * this.  Never more than next_pow2(min(la, out_len) + min(lb, out_len) - 1) for mul and next_pow2(2 L - 1) for inverse
 * (L = out_len) and div (L = la - lb + 1): the reference's own lengths (poly.rs:341, :109). */
size_t kzgamd_poly_transform_len(int op, size_t la, size_t lb, size_t out_len);
/* Zero polynomials and sample recovery, the reference's ZeroPoly and PolyRecover (kzg/src/lib.rs:433-463, 535-545;
 * blst/src/zero_poly.rs, blst/src/recovery.rs) on the poly handle (rust-kzg_amd/csrc/zeropoly.hip), with the conventions
 * of kzgamd_poly_*.  Positive codes are tested in the order listed; on a positive code nothing is written.  Every output
 * is a field element with one value — a monic product of linear factors, its transform, a pointwise quotient whose
 * divisor is never zero (5 is not a 2^k-th root of unity) — so results equal the reference's element for element.
 * roots[] below is the handle's roots_of_unity table (kzgamd_ntt_roots), max_width + 1 entries.
 *
 * kzgamd_poly_zero_partial: out[0 .. nidx] = the nidx + 1 coefficients of prod_k (X - roots[idxs[k] * stride]), lowest
 * first (do_zero_poly_mul_partial, for any nidx; repeated indices allowed).  1: nidx == 0, 2: some idxs[k] * stride >
 * max_width, 4: the product needs a transform longer than the max width. */
int kzgamd_poly_zero_partial(void *ph, blst_fr *out, const uint64_t *idxs, size_t nidx, size_t stride);
/* out = the sum(lens[k] - 1) + 1 coefficients of the product of npartial polynomials stored back to back in `partials`
 * (reduce_partials; any coefficients, monic or not).  1: domain_size is not a power of two, 2: npartial == 0,
 * 5: some lens[k] == 0, 3: out degree + 1 > domain_size, 4: domain_size > max width. */
int kzgamd_poly_reduce_partials(void *ph, blst_fr *out, size_t domain_size, const blst_fr *partials, const size_t *lens,
                                size_t npartial);
/* zero_poly_via_multiplication for nprob index lists in one call: problem b has missing[offsets[b] .. offsets[b+1]).
 * zero_poly[b * domain_size ..] = prod (X - w^idx), zero-padded to domain_size, w = roots[max_width / domain_size];
 * zero_eval[b * domain_size ..] = its forward transform.  Either output may be NULL.  1: a list has >= domain_size
 * entries, 2: domain_size > max width, 3: domain_size is not a power of two (0 included), 5: an index >= domain_size.
 * An empty list gives the empty product (zero_poly = 1, 0, 0, ...; zero_eval all ones); nprob = 0: ok, nothing
 * written.  form 0: chosen by shape, 1: direct (a lane per domain point multiplies out Z(w^t); one inverse transform),
 * 2: product tree (a wave per 64 roots, then one batched pair of transforms per level).  All forms give the same
 * elements. */
int kzgamd_poly_zero_poly(void *ph, blst_fr *zero_eval, blst_fr *zero_poly, size_t domain_size, const uint64_t *missing,
                          const size_t *offsets /* nprob + 1 */, size_t nprob, int form);
/* nprob sample vectors of n elements; present[b * n + i] == 0 marks a missing sample, whose value is never used.
 * coeffs != 0: recover_poly_coeffs_from_samples, coeffs == 0: recover_poly_from_samples.  Defined for any sample
 * values: with Z the zero polynomial of the missing set, E the samples with zeros in the gaps and s_k(p) the map
 * coefficient i -> p_i k^i (exponent i, NOT the i + 1 of kzgamd_poly_scale), the coefficient form is
 * s_5(ifft(fft(s_1/5(ifft(E . fft Z))) / fft(s_1/5(Z)))).  1: n is not a power of two (0 included), 2: a vector has more
 * than n / 2 missing, 3: n > max width.  No missing sample: ifft(samples), or the samples.  Any n up to the max width. */
int kzgamd_poly_recover(void *ph, blst_fr *out, const blst_fr *samples, const uint8_t *present, size_t n, size_t nprob,
                        int coeffs);
/* the roots a wave of the leaf kernel takes, and the largest list of a call for which form 0 of kzgamd_poly_zero_poly
 * (and kzgamd_poly_recover) takes the direct form (0 in this build: the tree measured level or ahead at every size, the
 * direct form is form 1 only); any pointer may be NULL */
int kzgamd_poly_zero_info(void *ph, size_t *leaf_roots, size_t *direct_max);
/* host-only, no GPU: the levels the tree form runs for `count` roots, levels[3 * l ..] = {polynomials entering the
 * level, coefficients of each below its leading 1 (the last may have fewer), transform length}.  Returns the number of
 * levels, ceil(log2(ceil(count / leaf_roots))), at most 32.  The longest transform is never more than next_pow2(count + 1). */
size_t kzgamd_poly_zero_plan(size_t count, size_t *levels /* 32 x 3 */);
/* The tile plan the NTT kernel runs for (kind, T) — host-only, no GPU needed (rust-kzg_amd/csrc/ntt_plan.h):
 * kind 0 = whole transform of 2^T <= 4096 points, 1 = first pass of a longer one, 2 = later pass; rounds[4*r..] =
 * {first stage, stages, barrier after, element bit}; tab[(r*1024 + thread)*4..] = {idxA, idxB, lds(idxA), lds(idxB)}.
 * Returns the number of rounds (<= 6), -1 on bad arguments. */
int kzgamd_ntt_plan_dump(int kind, int T, int *rounds /* 6 x 4 */, uint16_t *tab /* 6 x 1024 x 4 */);
/* The same for the one-pass DAS extension of lists of 2^T <= 4096 elements (inverse rounds, twist, forward rounds in
 * one tile): rounds[6*r..] = {first stage, stages, barrier after, element bit, flags (1 forward half, 2 unit
 * twiddles, 4 twist before the LDS store), LDS position bit of the element bit}.  Returns the rounds (<= 12). */
int kzgamd_ntt_das_plan_dump(int T, int *rounds /* 12 x 6 */, uint16_t *tab /* 12 x 1024 x 4 */);

/* ------------------------------------------------------------------------------------------
 * B3 — c-kzg-4844 surface for the proving path (blst/src/eip_4844.rs:160-530).
 * Types follow kzg/src/eth/c_bindings.rs:16-113.  Every failure maps to C_KZG_BADARGS like the
 * reference (blst/src/utils.rs:47-56).
 * ------------------------------------------------------------------------------------------ */
typedef enum { C_KZG_OK = 0, C_KZG_BADARGS = 1, C_KZG_ERROR = 2, C_KZG_MALLOC = 3 } C_KZG_RET;
#define BYTES_PER_BLOB 131072
#define FIELD_ELEMENTS_PER_BLOB 4096
typedef struct { uint8_t bytes[32]; } Bytes32;
typedef struct { uint8_t bytes[48]; } Bytes48;
typedef struct { uint8_t bytes[BYTES_PER_BLOB]; } Blob;
typedef Bytes48 KZGCommitment;
typedef Bytes48 KZGProof;

/* Same layout as the reference's CKZGSettings (kzg/src/eth/c_bindings.rs:55-108).  The host arrays are
 * owned by the library and freed by free_trusted_setup; the device-resident state (fixed-base MSM table)
 * is found through a registry keyed by g1_values_lagrange_brp, as the reference does for its tables
 * (kzg/src/eip_4844.rs:64-146).  tables / wbits / scratch_size stay empty like the reference's
 * (blst/src/eip_4844.rs:140-142). */
typedef struct {
    blst_fr *roots_of_unity;          /* 8193 */
    blst_fr *brp_roots_of_unity;      /* 8192 */
    blst_fr *reverse_roots_of_unity;  /* 8193 */
    blst_p1 *g1_values_monomial;      /* 4096 */
    blst_p1 *g1_values_lagrange_brp;  /* 4096 */
    blst_p2 *g2_values_monomial;      /* 65 */
    blst_p1 **x_ext_fft_columns;      /* 128 rows x 64 (FK20 columns, blst/src/types/kzg_settings.rs:84-101) */
    blst_p1_affine **tables;          /* NULL */
    size_t wbits;
    size_t scratch_size;
} CKZGSettings;

/* Exact c-kzg-4844 names and signatures, as exported by blst/src/eip_4844.rs. */
C_KZG_RET load_trusted_setup(CKZGSettings *out, const uint8_t *g1_monomial_bytes, uint64_t num_g1_monomial_bytes,
                             const uint8_t *g1_lagrange_bytes, uint64_t num_g1_lagrange_bytes,
                             const uint8_t *g2_monomial_bytes, uint64_t num_g2_monomial_bytes,
                             uint64_t precompute);                                             /* eip_4844.rs:180-222 */
C_KZG_RET load_trusted_setup_file(CKZGSettings *out, FILE *in);                                /* eip_4844.rs:227-269 */
void free_trusted_setup(CKZGSettings *s);                                                      /* eip_4844.rs:296-378 */
C_KZG_RET blob_to_kzg_commitment(KZGCommitment *out, const Blob *blob, const CKZGSettings *s); /* eip_4844.rs:163-175 */
C_KZG_RET compute_kzg_proof(KZGProof *proof_out, Bytes32 *y_out, const Blob *blob, const Bytes32 *z_bytes,
                            const CKZGSettings *s);                                            /* eip_4844.rs:476-496 */
C_KZG_RET compute_blob_kzg_proof(KZGProof *out, const Blob *blob, const Bytes48 *commitment_bytes,
                                 const CKZGSettings *s);                                       /* eip_4844.rs:274-291 */
/* Verification (eip_4844.rs:383-471).  The field work (challenge, evaluation) and, for batches, the G1 linear
 * combinations run on the GPU; the pairing check itself runs on the host, as in the reference (its GPU backend moves
 * only g1_lincomb; blst/src/kzg_proofs.rs:73-100 is CPU code).  *ok is the verdict; malformed input -> C_KZG_BADARGS. */
C_KZG_RET verify_kzg_proof(bool *ok, const Bytes48 *commitment_bytes, const Bytes32 *z_bytes, const Bytes32 *y_bytes,
                           const Bytes48 *proof_bytes, const CKZGSettings *s);                 /* eip_4844.rs:383-405 */
C_KZG_RET verify_blob_kzg_proof(bool *ok, const Blob *blob, const Bytes48 *commitment_bytes, const Bytes48 *proof_bytes,
                                const CKZGSettings *s);                                        /* eip_4844.rs:410-430 */
C_KZG_RET verify_blob_kzg_proof_batch(bool *ok, const Blob *blobs, const Bytes48 *commitments_bytes,
                                      const Bytes48 *proofs_bytes, size_t n, const CKZGSettings *s); /* eip_4844.rs:435-471 */
/* helpers the reference exports for the binding test-suites (eip_4844.rs:501-530) */
void compute_challenge(blst_fr *eval_challenge_out, const Blob *blob, const blst_p1 *commitment);
C_KZG_RET bytes_to_kzg_commitment(blst_p1 *out, const Bytes48 *b);
void bytes_from_bls_field(Bytes32 *out, const blst_fr *in);

/* Batched forms (new API; BASELINE.json configs[4] names a compute_blob_kzg_proof_batch the reference
 * does not have — its closest behaviour is a host loop, kzg-bench/src/benches/eip_4844.rs:56-60).
 * Per-blob results equal the single-blob calls; any invalid blob fails the whole call (BadArgs). */
C_KZG_RET kzgamd_blob_to_kzg_commitment_batch(KZGCommitment *out, const Blob *blobs, size_t n, const CKZGSettings *s);
C_KZG_RET kzgamd_compute_blob_kzg_proof_batch(KZGProof *out, const Blob *blobs, const Bytes48 *commitments, size_t n,
                                              const CKZGSettings *s);
/* Device-resident commit, enqueued on `stream` without synchronising: d_blobs = n x 131072 B,
 * d_out = n x 48 B, d_status = n x int32 (0 ok, 1 blob has an element >= r),
 * d_scratch = n x 131072 B of workspace. */
C_KZG_RET kzgamd_blob_to_kzg_commitment_device(void *d_out, void *d_status, void *d_scratch, const void *d_blobs,
                                               size_t n, const CKZGSettings *s, void *stream);
/* Device-resident compute_blob_kzg_proof (kzg/src/eip_4844.rs:541-584) for n blobs, enqueued on `stream` without
 * synchronising: d_blobs = n x 131072 B, d_commitments = n x 48 B, d_proofs = n x 48 B, d_status = n x int32
 * (non-zero: blob i has an element >= r or commitment i is not a valid G1 element — the reference fails the call;
 * here the other proofs of the batch stay valid), d_scratch = n x KZGAMD_PROOF_SCRATCH_BYTES of workspace.
 * The Fiat-Shamir SHA-256 runs on the device too (one lane per blob: ~9 ms of latency per batch and about a percent
 * of the chip — pipeline batches on a few streams); kzgamd_settings_reserve covers the MSM workspace. */
#define KZGAMD_PROOF_SCRATCH_BYTES (131072 + 64)
C_KZG_RET kzgamd_compute_blob_kzg_proof_device(void *d_proofs, void *d_status, void *d_scratch, const void *d_blobs,
                                               const void *d_commitments, size_t n, const CKZGSettings *s, void *stream);
/* EIP-7594: cells (128 x 2048 B) and cell proofs (128 x 48 B) of a blob, same name
 * and signature as the reference (kzg/src/eth/c_bindings.rs:356-372); either output may be NULL, not
 * both.  The first call that asks for proofs builds a second wide table over g1_values_monomial. */
/* compute_challenges_and_evaluate_polynomial (kzg/src/eip_4844.rs:690-719): the per-blob field work of
 * verify_blob_kzg_proof_batch (:736-832) — z_i = Fiat-Shamir challenge of (blob_i, commitment_i), y_i = p_i(z_i),
 * both 32-byte big-endian.  Commitments are validated (decode + subgroup) as validate_batched_input does.  The
 * pairing side (verify_kzg_proof_batch, :380-435) stays on the caller's CPU backend. */
C_KZG_RET kzgamd_compute_challenges_and_evaluate_batch(Bytes32 *zs_out, Bytes32 *ys_out, const Blob *blobs,
                                                       const Bytes48 *commitments, size_t n, const CKZGSettings *s);

/* verify_kzg_proof_batch (kzg/src/eip_4844.rs:380-435) up to the pairing: r = Fiat-Shamir scalar of the n tuples
 * (compute_r_powers, :328-378);  proof_lincomb = sum r^i proof_i;  rhs = sum r^i (C_i - [y_i]G) + sum r^i z_i proof_i.
 * Commitments and proofs are decoded and subgroup-checked on the GPU (validate_batched_input, :721-734), z_i / y_i must
 * be canonical (< r); any violation -> C_KZG_BADARGS.  The caller (its CPU backend) finishes with the one pairing check
 *     e(proof_lincomb, g2_values_monomial[1]) == e(rhs, G2_generator).
 * n == 0 yields two points at infinity.  kzgamd_verify_blob_kzg_proof_batch_g1 is verify_blob_kzg_proof_batch
 * (:736-832) up to the same point: it derives z_i, y_i from the blobs first. */
C_KZG_RET kzgamd_verify_kzg_proof_batch_g1(blst_p1 *proof_lincomb_out, blst_p1 *rhs_out, const Bytes48 *commitments,
                                           const Bytes32 *zs, const Bytes32 *ys, const Bytes48 *proofs, size_t n,
                                           const CKZGSettings *s);
C_KZG_RET kzgamd_verify_blob_kzg_proof_batch_g1(blst_p1 *proof_lincomb_out, blst_p1 *rhs_out, const Blob *blobs,
                                                const Bytes48 *commitments, const Bytes48 *proofs, size_t n,
                                                const CKZGSettings *s);

/* Host-only helpers over blst_p2 and the pairing (no GPU involved): pairings_verify = blst/src/kzg_proofs.rs:73-100
 * (1 if e(a1,a2) == e(b1,b2), 0 if not, -1 on NULL); uncompress = FsG2::from_bytes (0 ok, 1 invalid encoding /
 * not on the curve); mult takes a Montgomery blst_fr like G2Mul (blst/src/types/g2.rs:24-39). */
int kzgamd_pairings_verify(const blst_p1 *a1, const blst_p2 *a2, const blst_p1 *b1, const blst_p2 *b2);
/* The same check for many G1 pairs against two shared G2 points, ON THE GPU (the calling thread's current device), one
 * wave per check: ok[i] = e(a1[i], *a2) == e(b1[i], *b2), i < count, the verdicts of kzgamd_pairings_verify item by
 * item (a side with Z = 0 or an identity G2 point is skipped; two skipped sides give true).  Coordinates are canonical
 * (below p), as blst produces them: for a Z that is a non-zero multiple of p neither form is defined.  0 ok, -1 NULL argument,
 * -2 or -(100 + hipError_t) device errors.  count = 0: success, nothing written, the pointers are not looked at.
 * Thread-safe; the line tables of the G2 points are cached per (device, point); large counts run in slices of
 * kzgamd_pairing_info's slice_checks (may be NULL; returns 0). */
int kzgamd_pairings_verify_batch(bool *ok, const blst_p1 *a1, const blst_p2 *a2, const blst_p1 *b1, const blst_p2 *b2,
                                 size_t count);
int kzgamd_pairing_info(size_t *slice_checks);
int kzgamd_p2_uncompress(blst_p2 *out, const uint8_t in[96]);
void kzgamd_p2_compress(uint8_t out[96], const blst_p2 *in);
void kzgamd_p2_generator(blst_p2 *out);
void kzgamd_p2_mult(blst_p2 *out, const blst_p2 *in, const blst_fr *scalar);
void kzgamd_p2_add(blst_p2 *out, const blst_p2 *a, const blst_p2 *b);

/* Fixed-base batched scalar multiplication ON THE GPU, in G1 and in G2 (G1Mul::mul / G2Mul::mul of the reference,
 * kzg/src/lib.rs:138-140, 413-415, for many scalars and one base), and the trusted setups made of it.  Handle-less: the
 * calls run on the calling thread's current device (cfg->device, when cfg is given and names one), take host buffers
 * and are thread-safe.  Outputs are Jacobian with canonical coordinates; infinity is Z == 0 (all-zero), as everywhere.
 *
 * out[i] = scalars[i] * (*base), i < n; base == NULL: the generator.  Scalars are Montgomery blst_fr (as G1Mul/G2Mul take
 * them).  The base is a Jacobian point of the prime-order subgroup with any Z (Z == 0: every output is infinity).  The G1
 * base is tested (blst_p1_in_g1); a G2 base is the caller's responsibility, like every blst_p2 this library accepts
 * (kzgamd_p2_in_g2 tests one, kzgamd_g2_uncompress_batch with check_subgroup tests them as they are parsed): for
 * one outside the subgroup the outputs are still the multiples k_i * base of the curve's group law.
 * n == 0: success, nothing written, the pointers are not looked at.
 *
 * kzgamd_generate_trusted_setup is generate_trusted_setup of the reference (blst/src/utils.rs:16-37):
 * s = hash_to_bls_field(secret) (the 32 bytes as a big-endian integer mod r), g1_monomial[i] = [s^i]G1 (i < num_g1),
 * g2_monomial[j] = [s^j]G2 (j < num_g2), g1_lagrange = fft_g1(g1_monomial, inverse) in natural order, computed on the
 * device from the device-resident points through the NTT handle `ntt` (kzgamd_ntt_new; only the Lagrange form needs it,
 * and the call then runs on the handle's device).  The powers of s are computed on the device.  Any of the three outputs
 * may be NULL (not computed).  Both counts 0: success, nothing written.
 *
 * Return codes:  0 ok;  1 g1_lagrange wanted, but num_g1 is not a power of two or ntt is NULL;  2 num_g1 exceeds the NTT
 * handle's max width;  3 the G1 base is not in the subgroup;  -1 a needed pointer is NULL;  -2 or -(100 + hipError_t)
 * device errors (-2 also for a malformed cfg).
 * cfg may be NULL.  Its tuning string takes ONE key, of these calls alone and not listed by kzgamd_tuning_keys:
 * mul_slice=<outputs per slice of workspace: a power of two, at least 64>; any other key fails the call.
 * Memory the library keeps: the window tables of the two generators (1.5 MB of device memory together) are built at the
 * first call that needs them on a device and stay until the process ends; there is no call that frees them, and they
 * do not survive a hipDeviceReset by the application (do not reset a device these calls have run on).  Everything
 * else a call allocates is freed before it returns.
 * kzgamd_group_mul_info: the default slice and the window widths of the two tables (any pointer may be NULL; returns 0). */
int kzgamd_g1_mul_batch(blst_p1 *out, const blst_p1 *base, const blst_fr *scalars, size_t n, const KzgAmdConfig *cfg);
int kzgamd_g2_mul_batch(blst_p2 *out, const blst_p2 *base, const blst_fr *scalars, size_t n, const KzgAmdConfig *cfg);
int kzgamd_generate_trusted_setup(void *ntt, blst_p1 *g1_monomial, blst_p1 *g1_lagrange, blst_p2 *g2_monomial,
                                  size_t num_g1, size_t num_g2, const uint8_t secret[32], const KzgAmdConfig *cfg);
int kzgamd_group_mul_info(size_t *slice_points, int *g1_window_bits, int *g2_window_bits);

/* Batched point serialisation ON THE GPU: G1::from_bytes / to_bytes / is_valid, G2::from_bytes / to_bytes and
 * G1Affine::into_affines of the reference (kzg/src/lib.rs:89-99, 400-402, 255-265) for many points in one call.
 * Handle-less, as the calls above: the calling thread's current device (cfg->device, when cfg is given and names one),
 * host buffers, thread-safe, a stream per call.
 *
 * Format: ZCash-compressed, 48 bytes in G1 and 96 in G2 (x.c1 | x.c0), big-endian, the three flag bits on top, as
 * kzgamd_p2_uncompress / kzgamd_p2_compress and bytes_to_kzg_commitment read and write it.
 * Inputs of compress / to_affine: Jacobian points with canonical coordinates (below p), as blst produces them, any Z.
 * The identity is Z == 0 (all-zero limbs) whatever X and Y hold; it compresses to 0xc0 00 .. 00 and its affine form is
 * (0, 0), blst's affine infinity.
 * uncompress: out[i] has Z = 1 and canonical Montgomery coordinates; the identity is all-zero.  status[i] (status may be
 * NULL): 0 ok; 1 not a valid encoding (flag bits, a coordinate >= p, no point with that x); 2 on the curve but outside
 * the prime-order subgroup, given only when check_subgroup != 0 (G1: phi(P) == -[x^2]P; G2: psi(P) == [x]P).  An entry
 * whose status is not 0 is written all-zero.
 *
 * Return codes:  0 every point was accepted (compress / to_affine: done);  1 at least one point was refused, outputs
 * and statuses are written;  -1 a needed pointer is NULL;  -2 or -(100 + hipError_t) device errors (-2 also for a
 * malformed cfg).  n == 0: success, nothing written, the pointers are not looked at.
 * cfg may be NULL.  Its tuning string takes ONE key, of these calls alone and not listed by kzgamd_tuning_keys:
 * codec_slice=<points per slice of workspace: a power of two, at least 64>; any other key fails the call.  Counts above
 * the slice run slice by slice through one workspace; kzgamd_codec_info reports the default (may be NULL; returns 0).
 * Everything runs on the GPU for every n >= 1: a call costs a stream, its workspace, the copies and a launch whatever
 * n is, so a caller with ONE point is better served by the host helpers (kzgamd_p2_uncompress, kzgamd_p2_compress,
 * kzgamd_p2_in_g2, bytes_to_kzg_commitment).
 * kzgamd_p2_in_g2 is that subgroup test for one point on the host (no GPU involved): 1 the point is in G2 (the identity
 * included), 0 it is not, -1 NULL.  The point must be on the curve, as every decoded point is. */
int kzgamd_g1_compress_batch(uint8_t *out48, const blst_p1 *in, size_t n, const KzgAmdConfig *cfg);
int kzgamd_g1_to_affine_batch(blst_p1_affine *out, const blst_p1 *in, size_t n, const KzgAmdConfig *cfg);
int kzgamd_g1_uncompress_batch(blst_p1 *out, uint8_t *status, const uint8_t *in48, size_t n, int check_subgroup,
                               const KzgAmdConfig *cfg);
int kzgamd_g2_compress_batch(uint8_t *out96, const blst_p2 *in, size_t n, const KzgAmdConfig *cfg);
int kzgamd_g2_uncompress_batch(blst_p2 *out, uint8_t *status, const uint8_t *in96, size_t n, int check_subgroup,
                               const KzgAmdConfig *cfg);
int kzgamd_p2_in_g2(const blst_p2 *p);
int kzgamd_codec_info(size_t *slice_points);
/* Trusted-setup files of ANY size, host text around the calls above, in the layout load_trusted_setup_file reads (and
 * tests/golden/trusted_setup.txt has): the two counts, then the Lagrange G1 points in natural order, the G2 points and
 * the monomial G1 points; lowercase hex, one point per line.  cfg as above (codec_slice).
 * write compresses the three arrays on the GPU and writes the text to `out` (flushed, not closed).
 * read: on entry *num_g1 and *num_g2 are the capacities of the arrays, on return the counts of the file.  The points
 * are parsed on the GPU with the subgroup test on for all three arrays; whitespace as load_trusted_setup_file accepts
 * it.  Any of the three arrays may be NULL: that section is skipped (with all three NULL the call only reads the counts).
 * Return codes:  0 ok;  1 malformed text or a count that does not parse;  2 a capacity is too small (the counts are
 * still written, no point is);  3 a point was refused (such entries are all-zero, the others are written);
 * -1 a needed pointer is NULL;  -2 or -(100 + hipError_t) device errors, a malformed cfg, a failed write. */
int kzgamd_write_trusted_setup_file(FILE *out, const blst_p1 *g1_monomial, const blst_p1 *g1_lagrange,
                                    const blst_p2 *g2_monomial, size_t num_g1, size_t num_g2, const KzgAmdConfig *cfg);
int kzgamd_read_trusted_setup_file(FILE *in, blst_p1 *g1_monomial, blst_p1 *g1_lagrange, blst_p2 *g2_monomial,
                                   size_t *num_g1, size_t *num_g2, const KzgAmdConfig *cfg);

/* G2 linear combinations ON THE GPU, and the verification of a trusted setup made of them.  Handle-less, as the calls
 * above: the calling thread's current device (cfg->device, when cfg is given and names one), host buffers, thread-safe,
 * a stream per call.
 *
 * kzgamd_g2_lincomb: *out = sum_i scalars[i] * points[i], i < n.  Scalars are Montgomery blst_fr.  Points are Jacobian
 * with canonical coordinates and any Z; Z == 0 is the identity.  The output is Jacobian, canonical, all-zero for the
 * identity.  n == 0 gives the identity, and points and scalars are not looked at.  The points are the caller's
 * responsibility, like every blst_p2 this library accepts: for points outside the subgroup the result is still the sum
 * of the curve's group law, as in kzgamd_g2_mul_batch.  One lane per point walks the 256 bits of its scalar
 * (double-and-add); the terms are summed pairwise on the device.
 * Return codes:  0 ok;  -1 a needed pointer is NULL;  -2 or -(100 + hipError_t) device errors (-2 also for a malformed
 * cfg).  cfg may be NULL.  Its tuning string takes ONE key, of the calls of this block alone and not listed by
 * kzgamd_tuning_keys: lincomb_slice=<points per slice of workspace: a power of two, at least 64>; any other key fails
 * the call.  Counts above the slice run slice by slice through one workspace, and the slice sums are added.
 * kzgamd_g2_lincomb_info reports the default slice (may be NULL; returns 0).
 *
 * kzgamd_verify_trusted_setup: is (M, L, Q) = (g1_monomial, g1_lagrange, g2_monomial) a trusted setup: the powers of
 * ONE secret on both sides, from the two generators, and L the inverse transform of M (natural order, as
 * kzgamd_generate_trusted_setup returns it and a setup file stores it)?  L may be NULL: that check is not made, and
 * `ntt` is not needed.  With L, `ntt` is an NTT handle at least num_g1 wide, and the call runs on its device.
 * PRECONDITION: every point is in its prime-order subgroup.  Neither this call nor any other tests a blst_p1 / blst_p2
 * array handed over; kzgamd_read_trusted_setup_file and the uncompress_batch calls with check_subgroup test points as
 * they are parsed (the file form below goes through the former).
 * The challenge: r = hash_to_bls_field(seed) (the 32 bytes as a big-endian integer mod r, the rule of `secret` in
 * kzgamd_generate_trusted_setup); r == 0 is replaced by 1.  With seed == NULL the 32 bytes are
 *     SHA-256( "KZGAMD_VERIFY_SETUP_V1" (22 bytes, no terminator) | num_g1 as 8 bytes big-endian | num_g2 as 8 bytes
 *              big-endian | one byte: 1 with L, 0 without | M compressed, 48 bytes a point | L compressed, 48 bytes a
 *              point (with L only) | Q compressed, 96 bytes a point ),
 * so a setup cannot be chosen after its challenge.  A caller's seed must be one the maker of the setup could not know.
 * The checks, each a bit of *failed (failed may be NULL); all of them run, not only the first to fail:
 *     1   M[0] is the G1 generator and Q[0] is the G2 generator (as points, any Z)
 *     2   G1 powers:  e(B, Q[0]) == e(A, Q[1])  with A = sum_{i < num_g1 - 1} r^i M[i],  B = sum_{i < num_g1 - 1} r^i M[i + 1]
 *     4   G2 powers:  e(M[1], C) == e(M[0], D)  with C = sum_{j < num_g2 - 1} r^j Q[j],  D = sum_{j < num_g2 - 1} r^j Q[j + 1]
 *     8   Lagrange form:  sum_i f[i] L[i] == sum_k r^k M[k]  with f = ntt_fr(r^0 ... r^(num_g1 - 1)) (forward)
 * What passes is a setup except with probability at most (2 num_g1 + num_g2) / |Fr| over r.
 * Return codes:  0 every requested check passed;  1 at least one failed, *failed says which;  2 num_g1 < 2 or
 * num_g2 < 2;  3 L was given but num_g1 is not a power of two, ntt is NULL, or num_g1 exceeds the handle's width;
 * -1 a needed pointer is NULL;  -2 or -(100 + hipError_t) device errors or a malformed cfg (lincomb_slice, as above).
 *
 * kzgamd_verify_trusted_setup_file reads `in` with kzgamd_read_trusted_setup_file (subgroup test on, all three arrays)
 * and verifies what it read, L included.  That call's codes 1, 2, 3 come back as 11, 12, 13 (13: a point was refused,
 * which also covers a point outside its subgroup); otherwise the codes above. */
int kzgamd_g2_lincomb(blst_p2 *out, const blst_p2 *points, const blst_fr *scalars, size_t n, const KzgAmdConfig *cfg);
int kzgamd_g2_lincomb_info(size_t *slice_points);
int kzgamd_verify_trusted_setup(void *ntt, unsigned *failed, const blst_p1 *g1_monomial, const blst_p1 *g1_lagrange,
                                const blst_p2 *g2_monomial, size_t num_g1, size_t num_g2, const uint8_t seed[32],
                                const KzgAmdConfig *cfg);
int kzgamd_verify_trusted_setup_file(void *ntt, unsigned *failed, FILE *in, const uint8_t seed[32], const KzgAmdConfig *cfg);

/* A prepared bucket MSM in G2 ON THE GPU: many linear combinations over ONE fixed set of points (a setup [s^j]G2, a
 * ceremony transcript), singly or in batches.  A handle, thread-safe like every handle: calls on one handle take turns,
 * calls on different handles run beside each other.  Host buffers in and out.
 *
 * kzgamd_g2_msm_new: a handle over points[0 .. npoints) on the calling thread's current device (cfg->device, when cfg is
 * given and names one).  Points are Jacobian with canonical coordinates and any Z; Z == 0 is the identity, whatever X
 * and Y hold.  The points are the caller's responsibility, like every blst_p2 this library accepts: for points outside
 * the subgroup every result is still the sum under the curve's group law.  npoints == 0 is allowed (points may then be
 * NULL): every sum of such a handle is the identity.
 * What the handle keeps: the table 2^(8k) * points[i], k < 32, as affine points of 240 bytes, 7680 bytes per point
 * (kzgamd_g2_msm_info: table_bytes): 252 MB for 2^15 points, 8 GB for 2^20.  Creation doubles every point 248 times
 * and inverts 32 times per point on the GPU, 65536 points per launch, and needs 0.7 GB of workspace beside the table
 * while it runs.  Measured on an MI355X with the upload (2026-10-21, profiles/g2_msm_time.jsonl, median of 5): 6.3 ms at
 * 65 points, 6.5 ms at 2^12, 8.1 ms at 2^15, 140 ms at 2^20.
 * *err (err may be NULL):  0 ok;  2 the table would exceed cfg->table_budget_bytes (0: no cap but the memory that is
 * free);  -1 points is NULL with npoints > 0;  -2 a malformed cfg or an unknown tuning key;  other negatives: device
 * errors.  NULL is returned on any error, and nothing stays allocated.
 * cfg may be NULL.  Its tuning string takes TWO keys, of this call alone, read at creation only, not listed by
 * kzgamd_tuning_keys and not carried by the environment:
 *     g2msm_segment=<entries one lane accumulates: a power of two, at least 2>
 *     g2msm_pass_entries=<cap on the (point, window) entries sorted and accumulated in one pass: a multiple of 32, at
 *                         least 32; a call above the cap runs in several passes, and the pass results are added>
 * Any other key fails the creation with -2.
 *
 * kzgamd_g2_msm: out[b] = sum_{i < n} scalars[b * n + i] * points[i] for b < nbatch, n <= npoints: the first n points
 * are used, as kzgamd_kzg_commit treats len.  Scalars are Montgomery blst_fr.  Every output is Jacobian with Z = one and
 * canonical coordinates, or all-zero for the identity: the result of a call is one fixed byte string, whatever order
 * the device added the terms in.  n == 0 gives identities (out is still required when nbatch > 0); nbatch == 0
 * succeeds, nothing is written and no pointer is looked at.
 * Return codes:  0 ok;  1 n > npoints;  -1 a needed pointer is NULL;  -(100 + hipError_t) a device error.
 * Every scalar is recoded into 32 signed base-256 digits; every non-zero digit is one table point added into one of 128
 * buckets of its batch item (at most 32 mixed additions per point and no doubling, against 256 doublings and about 128
 * additions of kzgamd_g2_lincomb), and the buckets are summed with their indices as weights.
 * This call is the faster form from the smallest count measured, 65 points, and the recommended one wherever a point
 * set is used more than once.  Medians of 5, kzgamd_g2_msm / kzgamd_g2_lincomb on the same inputs in the same run
 * (2026-10-21, profiles/g2_msm_time.jsonl; the five runs of either call lie within 1.8 ms of each other at every count):
 * 1.7 / 17.8 ms at 65 points, 2.6 / 17.8 ms at 2^12, 3.6 / 18.5 ms at 2^15, 28.7 / 287 ms at 2^20; 16 vectors over 2^15
 * points 15.0 ms in one call against 297 ms in 16.  A handle used once pays its creation too: 8.0 / 17.8 ms at 65 points,
 * 11.7 / 18.5 ms at 2^15, 169 / 287 ms at 2^20, still ahead.  Counts below 65 were not measured.
 *
 * kzgamd_g2_msm_info: the shape of a handle (any pointer may be NULL): its points, the window width in bits, the two
 * tuning values and the bytes of its table.  0, or -1 for a NULL handle.
 * kzgamd_g2_msm_free gives back every byte of HBM; NULL is a no-op. */
void *kzgamd_g2_msm_new(const blst_p2 *points, size_t npoints, const KzgAmdConfig *cfg, int *err);
void kzgamd_g2_msm_free(void *h);
int kzgamd_g2_msm(void *h, blst_p2 *out, const blst_fr *scalars, size_t n, size_t nbatch);
int kzgamd_g2_msm_info(void *h, size_t *npoints, int *window_bits, size_t *segment, size_t *pass_entries, size_t *table_bytes);

typedef struct { uint8_t bytes[2048]; } Cell;
C_KZG_RET compute_cells_and_kzg_proofs(Cell *cells, KZGProof *proofs, const Blob *blob, const CKZGSettings *s);
C_KZG_RET kzgamd_compute_cells_and_kzg_proofs_batch(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n,
                                                    const CKZGSettings *s);
/* EIP-7594 recovery and cell verification (kzg/src/eth/c_bindings.rs:202-355 -> kzg/src/das.rs:101-243, 294-389).
 * recover: num_cells in [64, 128] cells with strictly ascending cell_indices < 128 -> all 128 cells and (unless
 * recovered_proofs is NULL) their 128 proofs; the five 8192-point transforms, coset shifts and inversions run on the GPU.
 * verify: ok = every (commitment, cell index, cell, proof) tuple is consistent; num_cells = 0 is true; decoding,
 * subgroup checks and the linear combinations (one two-row MSM) on the GPU, one pairing check on the host.
 * Every failure of the reference (bad encoding, element >= r, index >= 128, point outside G1, too few / unordered
 * cells) is C_KZG_BADARGS, as there. */
C_KZG_RET recover_cells_and_kzg_proofs(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                       const Cell *cells, uint64_t num_cells, const CKZGSettings *s);
/* n independent recoveries in one call, the result of n calls of recover_cells_and_kzg_proofs (das.rs:209-241).
 * Blob b gives num_cells[b] cells. Its indices and cells are the next num_cells[b] entries of cell_indices / cells
 * (concatenated in blob order). recovered_cells: n x 128 cells; recovered_proofs: n x 128 proofs, or NULL.
 * Each blob is validated as in the single call. On any failure: the code of the first failing blob, and the outputs
 * are unspecified. n = 0: C_KZG_OK. */
C_KZG_RET kzgamd_recover_cells_and_kzg_proofs_batch(Cell *recovered_cells, KZGProof *recovered_proofs,
                                                    const uint64_t *cell_indices, const Cell *cells,
                                                    const uint64_t *num_cells, size_t n, const CKZGSettings *s);
C_KZG_RET verify_cell_kzg_proof_batch(bool *ok, const Bytes48 *commitments_bytes, const uint64_t *cell_indices,
                                      const Cell *cells, const Bytes48 *proofs_bytes, uint64_t num_cells,
                                      const CKZGSettings *s);
/* kzgamd_verify_cell_kzg_proof_batch_many: nbatch independent verify_cell_kzg_proof_batch inputs in one call under ONE
 * pairing — the data-column sidecars of a slot, each with its own verdict.  Batch b owns the next num_cells[b] entries
 * of commitments_bytes / cell_indices / cells / proofs_bytes (concatenated in batch order, the convention of
 * kzgamd_recover_cells_and_kzg_proofs_batch).  For valid input ok_each[b] is what verify_cell_kzg_proof_batch returns
 * for batch b alone, and *ok is their conjunction.
 *   Inner challenges: r_b = compute_verify_cell_kzg_proof_batch_challenge of batch b alone (over its own de-duplicated
 *     commitments in order of first appearance; a batch of zero cells hashes its header only and contributes no points).
 *   Outer weights: rho_b = rho^b (rho_0 = 1).
 *     rho == NULL: rho = hash_to_bls_field(SHA-256("KZGAMD_VCELLSET1" (16 bytes) | u64_be(nbatch) | the nbatch r_b as
 *       canonical 32-byte big-endian scalars)) — the digest as a big-endian integer mod the group order;
 *     rho != NULL (Montgomery): used as given, for callers with a transcript of their own (and for tests).  Such a rho
 *       MUST be fixed after every input of the call is: a rho the prover can anticipate lets errors of different
 *       batches cancel (rho = 1 adds the batches up unweighted, rho = 0 checks batch 0 alone).
 *   With (P_b, L_b) the reference's pair of batch b (proof_lincomb and the right-hand side, das.rs:294-389):
 *     P = sum rho_b P_b,   L = sum rho_b L_b,   *ok = e(L, G2) == e(P, [s^64]G2).
 * One call makes one set of uploads, one aggregated interpolation polynomial (sum_b rho_b I_b is 64 coefficients: the
 * outer weights are folded into the cell weights rho_b r_b^i), one two-row MSM over [all proofs | the commitments
 * de-duplicated across the call | g1_monomial[0..64)] and one download; the r_b are hashed on up to 8 host threads
 * meanwhile.  The cells go to the GPU as passed and are range-checked there.
 * ok_each (may be NULL): when the combined check passes every entry is true; when it fails the entries are
 * verify_cell_kzg_proof_batch's, batch by batch (nbatch more pairings: the slow path, taken only on failure).
 * Anything the single call rejects, in any batch (index >= 128, cell element >= r, bad G1 encoding, proof or
 * commitment outside G1), and a NULL argument, is C_KZG_BADARGS with nothing written.  nbatch = 0: *ok = true (the
 * input arrays are not looked at); batches without cells are true.
 * kzgamd_verify_cell_kzg_proof_batch_many_g1: out[0] = P, out[1] = L (Jacobian) of the same inputs and the same rho, no
 * pairing, for callers that pair themselves; nbatch = 0, or no cells at all: two identities.
 * kzgamd_vcells_info: the number of cells one wave of the aggregation kernel sums (a column with more is cut into
 * slices of that many); returns 0.
 * kzgamd_vcells_timing: host wall-clock milliseconds of the stages of the last _many / _many_g1 call on `s` that
 * reached the GPU, for measurements (tools/time_verify_cells_many.py): [0] de-duplication and staging until the decode
 * is enqueued, [1] handing the cells to the copy engine, [2] until every r_b is hashed (from the same start as [1]: the
 * upload and the table building run beside the hashes), [3] rho, weights and row scalars, [4] the aggregation kernels
 * to the 64 coefficients, [5] the two-row MSM with the wait for the decode, [6] the pairing, [7] the per-batch fallback
 * (0 when not taken; [6] and [7] are _many's).  0 ok, -1 NULL argument or unknown settings. */
C_KZG_RET kzgamd_verify_cell_kzg_proof_batch_many(bool *ok, bool *ok_each, const Bytes48 *commitments_bytes,
                                                  const uint64_t *cell_indices, const Cell *cells,
                                                  const Bytes48 *proofs_bytes, const uint64_t *num_cells, size_t nbatch,
                                                  const blst_fr *rho, const CKZGSettings *s);
C_KZG_RET kzgamd_verify_cell_kzg_proof_batch_many_g1(blst_p1 out[2], const Bytes48 *commitments_bytes,
                                                     const uint64_t *cell_indices, const Cell *cells,
                                                     const Bytes48 *proofs_bytes, const uint64_t *num_cells, size_t nbatch,
                                                     const blst_fr *rho, const CKZGSettings *s);
int kzgamd_vcells_info(size_t *slice_cells);
int kzgamd_vcells_timing(const CKZGSettings *s, double ms[8]);
/* blst/src/eip_7594.rs:35-97: the Fiat-Shamir scalar of a cell batch over DEDUPLICATED commitments (Montgomery blst_fr) */
C_KZG_RET compute_verify_cell_kzg_proof_batch_challenge(blst_fr *challenge_out, const Bytes48 *commitment_bytes,
                                                        uint64_t num_commitments, const uint64_t *commitment_indices,
                                                        const uint64_t *cell_indices, const Cell *cells,
                                                        const Bytes48 *proofs_bytes, uint64_t num_cells);
/* load_trusted_setup / load_trusted_setup_file with a configuration (device, table budget, tuning); same outputs and
 * failures, plus C_KZG_BADARGS for a malformed configuration */
C_KZG_RET kzgamd_load_trusted_setup_ex(CKZGSettings *out, const uint8_t *g1_monomial_bytes, uint64_t num_g1_monomial_bytes,
                                       const uint8_t *g1_lagrange_bytes, uint64_t num_g1_lagrange_bytes,
                                       const uint8_t *g2_monomial_bytes, uint64_t num_g2_monomial_bytes,
                                       uint64_t precompute, const KzgAmdConfig *cfg);
C_KZG_RET kzgamd_load_trusted_setup_file_ex(CKZGSettings *out, FILE *in, const KzgAmdConfig *cfg);
/* the prepared-MSM handle behind a settings object (for kzgamd_msm_* calls) */
void *kzgamd_settings_msm_handle(const CKZGSettings *s);
/* the GPU a settings object lives on (-1 if unknown) */
int kzgamd_settings_device(const CKZGSettings *s);
/* pre-allocates the per-stream workspace kzgamd_blob_to_kzg_commitment_device needs for batches of up to n blobs
 * on `stream` (see kzgamd_msm_reserve) */
C_KZG_RET kzgamd_settings_reserve(const CKZGSettings *s, size_t n, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU from ONE process, inside the library (rust-kzg_amd/csrc/multi.hip).  The reference's callers are
 * one Rust process that parallelises inside itself over groups of blobs (kzg/src/eip_4844.rs:770-816) around one shared
 * precomputation handle (kzg/src/msm/sppark.rs:24-44); its GPU path is single-device
 * (arkworks3-sppark-wlc/sppark/msm/pippenger.cuh:573-575).  Here: s[0..ndev) are settings objects loaded from the
 * same trusted setup, normally one per GPU (two on one GPU work too — with a table budget that lets both fit — and are how the
 * path is tested on a one-GPU box).  Blob i of the batch goes to s[k] for the k with lo_k <= i < hi_k, contiguous slabs
 * whose sizes differ by at most one; one host thread per settings object drives that object's single-device pipeline;
 * results land in place in out[].  Nothing is exchanged between devices (no collective): blobs are independent and
 * every device has its own replica of the tables.  Per-blob results equal the single-device calls; any failing slab
 * fails the call (C_KZG_BADARGS, like the reference).  n < ndev uses the first n objects.
 * ------------------------------------------------------------------------------------------ */
/* the slab [*lo, *hi) of part k when n items are cut into `parts` contiguous slabs whose sizes differ by at most one
 * (what every *_multi entry point uses; with n < parts the first n parts get one item).  Returns 0, 1 on bad arguments.
 * No GPU involved. */
int kzgamd_shard_range(size_t n, size_t parts, size_t k, size_t *lo, size_t *hi);
/* one CKZGSettings per entry of devices[] (NULL = GPUs 0 .. ndev-1) from one setup file, loaded in parallel; all or
 * nothing: on failure every out[d] is left empty.  The caller's current device is left alone. */
C_KZG_RET kzgamd_load_trusted_setup_file_multi(CKZGSettings out[], const int devices[], size_t ndev, FILE *in);
/* Page-locks (hipHostRegister, portable across devices) / releases a caller's buffer: copies between it and any device
 * are then direct DMA instead of passing through the runtime's staging of pageable memory (one CPU pass over the data
 * per device less — with several GPUs fed from one process that staging shares the host's memory bandwidth).  Optional:
 * every entry point takes pageable buffers.  0 ok, 1 failed (nothing changed). */
int kzgamd_pin_host_buffer(void *p, size_t bytes);
int kzgamd_unpin_host_buffer(void *p);
/* the same with a configuration for every object (cfg->device is ignored: devices[] places them); two objects on one
 * GPU need an explicit table_budget_bytes that lets both fit */
C_KZG_RET kzgamd_load_trusted_setup_file_multi_ex(CKZGSettings out[], const int devices[], size_t ndev, FILE *in,
                                                  const KzgAmdConfig *cfg);
void kzgamd_free_trusted_setup_multi(CKZGSettings s[], size_t ndev);
C_KZG_RET kzgamd_blob_to_kzg_commitment_batch_multi(KZGCommitment *out, const Blob *blobs, size_t n,
                                                    const CKZGSettings *const s[], size_t ndev);
C_KZG_RET kzgamd_compute_blob_kzg_proof_batch_multi(KZGProof *out, const Blob *blobs, const Bytes48 *commitments, size_t n,
                                                    const CKZGSettings *const s[], size_t ndev);
C_KZG_RET kzgamd_compute_cells_and_kzg_proofs_batch_multi(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n,
                                                          const CKZGSettings *const s[], size_t ndev);
/* the reference verifies a large batch as groups and ANDs the verdicts (kzg/src/eip_4844.rs:770-816); the groups here
 * are the devices' slabs: one pairing check per device */
C_KZG_RET kzgamd_verify_blob_kzg_proof_batch_multi(bool *ok, const Blob *blobs, const Bytes48 *commitments,
                                                   const Bytes48 *proofs, size_t n, const CKZGSettings *const s[],
                                                   size_t ndev);
/* One large MSM sharded by index range: msm[d] was prepared (prepare_msm after kzgamd_set_device(d), or
 * kzgamd_msm_create_device) over points[offsets[d] .. offsets[d+1]); scalars is the whole array (offsets[ndev]
 * elements, Montgomery blst_fr as mult_pippenger_prepared).  Every device sums its slice, the ndev 144-byte partials are
 * added on the host (kzgamd_g1_sum).  An empty slice (offsets[d] == offsets[d+1]) may have a NULL handle. */
RustError kzgamd_mult_pippenger_prepared_multi(void *const msm[], size_t ndev, blst_p1 *out, const size_t offsets[],
                                               const blst_fr scalars[]);

/* Multi-GPU combine step of one large MSM sharded by index range over G ranks: every rank computes
 * its partial with mult_pippenger / the device entry points over its slice of (points, scalars); the G
 * 144-byte Jacobian partials are all-gathered and summed locally with this host-side helper (a G1 addition is
 * not a reduction operator RCCL offers).  The reference has no multi-GPU path; its single-GPU call is
 * blst/src/kzg_proofs.rs:47-61. */
void kzgamd_g1_sum(blst_p1 *out, const blst_p1 in[], size_t n);

/* library / device info */
int kzgamd_device_count(void);
/* Multi-GPU from one process (the reference's sppark path is single-GPU, blst/src/kzg_proofs.rs:47-61).
 * kzgamd_set_device selects the GPU for the calling thread (hipSetDevice): handles created afterwards — prepare_msm,
 * kzgamd_msm_create_device, kzgamd_ntt_new, load_trusted_setup(_file) — live on that GPU.  Every later call on a
 * handle, host-buffer or device-resident form, switches to the handle's GPU by itself and restores the caller's
 * current device on return; device pointers and streams passed to a *_device entry point must belong to the
 * handle's GPU.  kzgamd_set_device returns 0, or 1 if the runtime refuses the index; kzgamd_get_device returns the
 * calling thread's current device, -1 on error. */
int kzgamd_set_device(int device);
int kzgamd_get_device(void);
/* What a settings object got of the HBM-sized tables it asked for (they are built on first use and shrink, or are left
 * out, when HBM is short — e.g. a second CKZGSettings on the same GPU): for which = 0 the commitment / proof table
 * over g1_values_lagrange_brp, 1 the cell-proof table of single blobs over g1_values_monomial, 2 the FK20 table over
 * x_ext_fft_columns — window bits, rows and the kzgamd_msm_uses_wide_table() code of the handle (0 = no wide table:
 * the bucket engine / the direct form runs instead; results are the same, only slower).  Returns 0, 1 when that
 * table has not been built (yet), -1 on bad arguments. */
int kzgamd_settings_table_info(const CKZGSettings *s, int which, int *window_bits, int *rows, int *wide_table);
const char *kzgamd_version(void);

#ifdef __cplusplus
}
#endif
#endif
