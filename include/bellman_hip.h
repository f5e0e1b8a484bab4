/*
 * bellman_hip.h -- C ABI of the MI355X-native Groth16 prover core.
 *
 * Drop-in boundary for the data-parallel hot path of doubiliu/bellman-mpc
 * (a fork of zkcrypto bellman 0.11.1).  Every entry point names the reference
 * interface it replaces (paths relative to bellman/src in the reference):
 *
 *   bh_multiexp            multiexp::multiexp            multiexp.rs:252-281
 *   bh_srs_upload          (Arc<Vec<G>>, usize) SourceBuilder / Parameters::read
 *                                                         multiexp.rs:45-86, groth16/mod.rs:292-400
 *   bh_fft / bh_ifft / bh_coset_fft / bh_icoset_fft /
 *   bh_distribute_powers / bh_divide_by_z_on_coset /
 *   bh_mul_assign / bh_sub_assign
 *                          EvaluationDomain methods      domain.rs:81-189
 *   bh_domain_size         EvaluationDomain::from_coeffs  domain.rs:47-79
 *   bh_evdom_*             EvaluationDomain with its coefficients resident in HBM
 *                                                         domain.rs:21-190
 *   bh_compute_h           the H block of create_proof   groth16/prover.rs:210-231
 *   bh_params_*            Parameters / ParameterSource  groth16/mod.rs:224-477
 *   bh_prove / bh_prove_witness
 *                          create_proof after synthesis   groth16/prover.rs:206-349
 *   bh_r1cs_*              KeypairAssembly                groth16/generator.rs:44-156
 *   bh_generate_parameters generate_parameters            groth16/generator.rs:241-634
 *   bh_srs_mul_each / _mul_powers / _sub_range
 *                          make_new_tau_paramter, matrixed_h groth16/mpc.rs:677-706, 631-635
 *   bh_mpc_common_*        the "common" ceremony round    groth16/mpc.rs:362-414, 708-862
 *   bh_mpc_uncommon_*      the "uncommon" ceremony round  groth16/mpc.rs:891-1131
 *   bh_srs_fft             EvaluationDomain<Point<G>>::fft / ifft   domain.rs:81-99, 192-228
 *   bh_mpc_common_matrix   CommonParamterInStorage::matrix, for any circuit   groth16/mpc.rs:597-645
 *   bh_mpc_parameters      generate_parameters_mpc        groth16/generator.rs:163-237
 *   bh_mpc_common_check / _verify_structure
 *                          the power-sequence check of a round-one storage (not in the reference)
 *   bh_params_check        Parameters against a circuit and such a storage (not in the reference;
 *                          the queries it audits: groth16/generator.rs:520-572, 614-633)
 *
 * Conventions
 *   - Plain pointers and sizes only; the caller owns every host buffer and the
 *     library never retains a caller pointer after a call returns -- except the inputs of
 *     bh_compute_h_scalars and bh_evdom_from_coeffs / bh_evdom_write, read asynchronously
 *     until the sync named there.
 *   - Fr vectors ("Montgomery") use the bls12_381 0.6 in-memory layout:
 *     4 little-endian u64 limbs of x * 2^256 mod r per element.
 *   - Exponents for bh_multiexp are Scalar::to_le_bits() words (canonical,
 *     4 LE u64 per scalar) unless BH_SCALARS_MONTGOMERY is given.  A canonical word
 *     >= r is taken mod r (the reference walks all 256 bits; k*P = (k mod r)*P in the
 *     prime-order group, so results agree).
 *   - Density maps are bitvec<u64, Lsb0> words: bit i of word i/64 is entry i.
 *   - Group elements use the zcash/bls12_381 encodings (big-endian, flag bits
 *     in byte 0): uncompressed 96 B (G1) / 192 B (G2), compressed 48/96 B.
 *   - Every function returns a bh_status; it never aborts across the FFI.
 *   - Process-wide side effect at load: GPU_MAX_HW_QUEUES is raised to 16 when it is
 *     unset or lower (HIP's default is 4; the prover keeps up to 12 streams busy and
 *     streams sharing a hardware queue serialise).  An explicitly set lower value is
 *     overridden too, with one line on stderr; BH_KEEP_HW_QUEUES=1 keeps the environment's
 *     value.  This only takes effect when the library loads before the first HIP call of
 *     the process.  Queue budget per context: DESIGN.md section 5.
 *   - bh_multiexp_submit jobs outlive nothing: destroying their context detaches every
 *     job not yet waited for, whose bh_multiexp_wait then returns BH_ERR_INVALID_ARGUMENT.
 */
#ifndef BELLMAN_HIP_H
#define BELLMAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes mirror SynthesisError (lib.rs:355-364). */
typedef int bh_status;
#define BH_OK 0
#define BH_ERR_UNEXPECTED_IDENTITY 1     /* multiexp.rs:63-65, prover.rs:309-313 */
#define BH_ERR_UNEXPECTED_EOF 2          /* IoError(UnexpectedEof), multiexp.rs:55-61,74-80 */
#define BH_ERR_POLY_DEGREE_TOO_LARGE 3   /* domain.rs:57-59 */
#define BH_ERR_DENSITY_SIZE_MISMATCH 4   /* the reference panics (assert), multiexp.rs:277 */
#define BH_ERR_UNCONSTRAINED_VARIABLE 5  /* generator.rs:582-586 */
#define BH_ERR_INVALID_ARGUMENT 10
#define BH_ERR_INVALID_ENCODING 11       /* IoError(InvalidData) of Parameters::read */
#define BH_ERR_NOT_ON_CURVE 12          /* the checked decoders' InvalidData (mod.rs:292-400) */
#define BH_ERR_NOT_IN_SUBGROUP 14       /* same reference error: not torsion-free */
#define BH_ERR_OUT_OF_MEMORY 13
#define BH_ERR_SCRATCH_LIMIT 15          /* a kernel's spill scratch would exceed the device's limit (no reference counterpart) */
#define BH_ERR_PAIRING_DEGENERATE 16     /* the device Miller loop met a zero denominator: a twist point outside the order-r subgroup (no reference counterpart) */
#define BH_ERR_HIP 100                  /* HIP runtime / device failure */

#define BH_G1 1
#define BH_G2 2

#define BH_SCALARS_CANONICAL 0
#define BH_SCALARS_MONTGOMERY 1

typedef struct bh_ctx bh_ctx;         /* one MI355X device + streams + workspaces (multicore.rs Worker) */
typedef struct bh_srs bh_srs;         /* device-resident affine base vector */
typedef struct bh_params bh_params;   /* device-resident Groth16 Parameters */
typedef struct bh_witness bh_witness; /* device-resident complete assignment */

const char* bh_status_string(bh_status s);
int bh_version(void);

/* ---- context (replaces multicore::Worker, multicore.rs:21-130) */
bh_status bh_ctx_create(int device, bh_ctx** out);
bh_status bh_ctx_destroy(bh_ctx* ctx);
/* Pre-allocate workspaces for MSMs up to max_msm_len and domains up to 2^max_log_domain,
 * so that later calls allocate nothing. */
bh_status bh_ctx_reserve(bh_ctx* ctx, size_t max_msm_len, uint32_t max_log_domain);
/* Force a window size for device MSMs (0 = automatic). Results never depend on it.
 * A forced window also disables the prover's window tables. */
bh_status bh_ctx_set_window(bh_ctx* ctx, int c);
/* Prover SRS window tables (default 1 = on): for each large query of the Parameters the
 * prover keeps T[i*W + w] = 2^(c*w) * P_i resident in HBM (built once per Parameters,
 * ~31 GB at 2^22 constraints on one GPU, 1/N of that per rank of an N-GPU run; skipped, with
 * a message on stderr, when HBM is short) so that all digit windows share one bucket set and
 * c can grow.  Results never depend on it. */
bh_status bh_ctx_set_tables(bh_ctx* ctx, int enable);

/* ---- bases (Source over Arc<Vec<G1Affine|G2Affine>>) */
bh_status bh_srs_upload(bh_ctx* ctx, int group, const uint8_t* uncompressed_be, size_t n, int checked,
                        bh_srs** out);
bh_status bh_srs_free(bh_srs* srs);
size_t bh_srs_len(const bh_srs* srs);
/* read back base i as uncompressed bytes (96/192 B) */
bh_status bh_srs_get(const bh_srs* srs, size_t i, uint8_t* out);
/* the same for bases first .. first + n in one copy: out receives n * 96 (192) bytes */
bh_status bh_srs_read(const bh_srs* srs, size_t first, size_t n, uint8_t* out);
/* The compressed half of the encodings (48 B G1: x; 96 B G2: x.c1 then x.c0; the compression flag,
 * the infinity flag and the sort flag = lex_largest(y) in the top bits of byte 0), coded on the
 * device one lane per point.
 *   bh_srs_upload_compressed  n compressed points -> a bh_srs that is word for word the one
 *                             bh_srs_upload builds from the same points' uncompressed bytes.  A
 *                             compressed point does not exist until it is decoded, so the flags, the
 *                             range of every coordinate and the squareness of x^3 + b are ALWAYS
 *                             checked, whatever `checked` is: any failing point gives
 *                             BH_ERR_INVALID_ENCODING (the compression flag clear; an infinity flag
 *                             with the sort flag or any other bit set; a coordinate >= p -- G2: c1
 *                             under the flags, and c0; x^3 + b not a square).  checked adds the
 *                             subgroup test only: BH_ERR_NOT_IN_SUBGROUP when every point decodes and
 *                             one is outside.  BH_ERR_NOT_ON_CURVE cannot arise.  The valid infinity
 *                             encoding (c0 00 ... 00) is accepted as bh_srs_upload accepts the
 *                             uncompressed one.  n = 0 gives an empty vector; argument errors as
 *                             bh_srs_upload.
 *   bh_srs_read_compressed    bases first .. first + n as compressed bytes: out receives n * 48 (96)
 *                             bytes; argument errors as bh_srs_read. */
bh_status bh_srs_upload_compressed(bh_ctx* ctx, int group, const uint8_t* compressed_be, size_t n, int checked,
                                   bh_srs** out);
bh_status bh_srs_read_compressed(const bh_srs* srs, size_t first, size_t n, uint8_t* out);
/* The uncompressed vector paths (bh_srs_upload, bh_srs_read, the vectors of bh_params_load / _write
 * and of the ceremony's uncompressed readers and writers) are coded on the device as well, one lane
 * per point: they replace the per-point loops of G1Affine / G2Affine::
 * from_uncompressed and into_uncompressed (groth16/mod.rs:260-400).  BH_POINT_CODEC_HOST=1 in the
 * environment, read at each call, keeps the host loops instead (an A/B and diagnostic mode; bytes and
 * statuses do not depend on it).  bh_srs_last_codec_device: 1 when the calling thread's last
 * uncompressed vector upload or read ran on the device codec, 0 when it ran on the host loops. */
int bh_srs_last_codec_device(void);

/* ---- multiexp::multiexp.  density_words == NULL means FullDensity.  out: uncompressed
 * encoding of the projective result normalised to affine (96 B for G1, 192 B for G2). */
bh_status bh_multiexp(bh_ctx* ctx, const bh_srs* bases, size_t base_offset, const uint64_t* density_words,
                      size_t density_len, const uint64_t* exponents, size_t n, int scalar_format, uint8_t* out);

/* ---- asynchronous multiexp: multiexp::multiexp returns a Waiter (multiexp.rs:252-281,
 * multicore.rs:94-110) and create_proof keeps eight in flight (prover.rs:233-307).  submit
 * enqueues the multiexp on a stream and workspace of its own and returns without waiting for
 * the device (the exponents and density words are read before it returns); wait blocks on
 * the job's event, writes the result like bh_multiexp and frees the job.  EOF / identity
 * errors of the Source are reported by wait, as the reference reports them from wait().
 * Thread-safe: any number of jobs per context, submitted and waited from any threads. */
typedef struct bh_job bh_job;
bh_status bh_multiexp_submit(bh_ctx* ctx, const bh_srs* bases, size_t base_offset, const uint64_t* density_words,
                             size_t density_len, const uint64_t* exponents, size_t n, int scalar_format,
                             bh_job** out);
bh_status bh_multiexp_wait(bh_job* job, uint8_t* out);

/* ---- the same seam on device-resident data.  create_proof clones one Arc<Vec<Fr::Repr>> per
 * assignment into several multiexps (prover.rs:233-307) and builds h into another
 * (prover.rs:227-231): a bh_scalars is that Arc on the device -- uploaded once (canonical or
 * Montgomery words, like bh_multiexp), or produced by bh_compute_h_scalars -- and any number of
 * multiexps read it.  bh_compute_h_scalars returns at once: a host thread uploads a, b, c and
 * enqueues the H passes, and multiexps submitted on h meanwhile are enqueued by that thread
 * behind them, so a caller can submit in create_proof's own order (h first) without waiting.  That
 * deferral is for submits on the producing context; a submit on another context of the device
 * first waits (on the host) until the producer has enqueued H, then enqueues normally.  Freeing the
 * handle is allowed while multiexps on it are in flight (they keep the device vector until their
 * wait). */
typedef struct bh_scalars bh_scalars;
bh_status bh_scalars_upload(bh_ctx* ctx, const uint64_t* exponents, size_t n, int scalar_format, bh_scalars** out);
bh_status bh_compute_h_scalars(bh_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                               size_t num_constraints, bh_scalars** h_out);
size_t bh_scalars_len(const bh_scalars* s);
bh_status bh_scalars_free(bh_scalars* s);
/* bh_compute_h_scalars reads a, b, c from a host thread of its own: they stay borrowed until this
 * returns (or a multiexp on the vector has been waited, or the vector is freed).  Returns the
 * H block's status (also reported by every multiexp waited on it). */
bh_status bh_scalars_sync(bh_scalars* s);
/* Profile of bh_compute_h_scalars' producer (waits like bh_scalars_sync), ms since the call:
 * [0..3) the copies of a, b, c enqueued, [3] the H passes enqueued, [4] the multiexps deferred
 * behind it enqueued, [5] how many were deferred.  A vector from bh_scalars_upload reports -1s. */
bh_status bh_scalars_stamps(bh_scalars* s, double out[6]);
bh_status bh_multiexp_submit_scalars(bh_ctx* ctx, const bh_srs* bases, size_t base_offset,
                                     const uint64_t* density_words, size_t density_len, const bh_scalars* exps,
                                     bh_job** out);

/* ---- EvaluationDomain.  Arrays hold 2^log_m Montgomery Fr (4 u64 each), in place. */
bh_status bh_domain_size(size_t len, size_t* m, uint32_t* log_m);
bh_status bh_fft(bh_ctx* ctx, uint64_t* coeffs, uint32_t log_m);
bh_status bh_ifft(bh_ctx* ctx, uint64_t* coeffs, uint32_t log_m);
bh_status bh_coset_fft(bh_ctx* ctx, uint64_t* coeffs, uint32_t log_m);
bh_status bh_icoset_fft(bh_ctx* ctx, uint64_t* coeffs, uint32_t log_m);
bh_status bh_distribute_powers(bh_ctx* ctx, uint64_t* coeffs, size_t len, const uint64_t g_mont[4]);
bh_status bh_divide_by_z_on_coset(bh_ctx* ctx, uint64_t* coeffs, uint32_t log_m);
bh_status bh_mul_assign(bh_ctx* ctx, uint64_t* a, const uint64_t* b, size_t len);
bh_status bh_sub_assign(bh_ctx* ctx, uint64_t* a, const uint64_t* b, size_t len);
/* ---- EvaluationDomain with its coefficients resident in HBM (domain.rs:21-190).  The
 * reference keeps `coeffs` private behind AsRef/AsMut/into_coeffs (domain.rs:21-45), so a
 * binding can hold them on the device from from_coeffs to into_coeffs: each method below is
 * an enqueue on the context's stream, and only bh_evdom_read / bh_evdom_into_scalars move
 * data back.  A handle belongs to its context (free it before the context) and is used by one
 * thread at a time (the reference's &mut self); different handles of one context may be used
 * from different threads.
 *   bh_evdom_from_coeffs   EvaluationDomain::from_coeffs   domain.rs:47-79 (zero-padded to 2^exp;
 *                          BH_ERR_POLY_DEGREE_TOO_LARGE past 2^31).  `coeffs` (len Montgomery Fr, 4 u64
 *                          each) is read asynchronously by the context's upload thread, in call
 *                          order: it stays borrowed until bh_evdom_sync (or read / into_scalars /
 *                          free) returns
 *   bh_evdom_fft / _ifft / _coset_fft / _icoset_fft      domain.rs:81-127
 *   bh_evdom_distribute_powers                           domain.rs:101-113
 *   bh_evdom_divide_by_z_on_coset                        domain.rs:139-151
 *   bh_evdom_mul_assign / _sub_assign                    domain.rs:153-189 (lengths must agree:
 *                          BH_ERR_INVALID_ARGUMENT, where the reference asserts)
 *   bh_evdom_read          as_ref / into_coeffs: the first len (<= m) coefficients, Montgomery
 *   bh_evdom_write         as_mut written back: replaces the coefficients by len (<= m) values,
 *                          zero-padded (asynchronous like from_coeffs)
 *   bh_evdom_into_scalars  prover.rs:226-231: the first len (<= m) coefficients as canonical
 *                          scalars (to_le_bits) in a device vector for bh_multiexp_submit_scalars,
 *                          without leaving the device; consumes the domain (later calls fail with
 *                          BH_ERR_INVALID_ARGUMENT, free still required) */
typedef struct bh_evdom bh_evdom;
bh_status bh_evdom_from_coeffs(bh_ctx* ctx, const uint64_t* coeffs, size_t len, bh_evdom** out);
bh_status bh_evdom_size(const bh_evdom* d, size_t* m, uint32_t* log_m);
bh_status bh_evdom_fft(bh_evdom* d);
bh_status bh_evdom_ifft(bh_evdom* d);
bh_status bh_evdom_coset_fft(bh_evdom* d);
bh_status bh_evdom_icoset_fft(bh_evdom* d);
bh_status bh_evdom_distribute_powers(bh_evdom* d, const uint64_t g_mont[4]);
bh_status bh_evdom_divide_by_z_on_coset(bh_evdom* d);
bh_status bh_evdom_mul_assign(bh_evdom* d, bh_evdom* other);
bh_status bh_evdom_sub_assign(bh_evdom* d, bh_evdom* other);
bh_status bh_evdom_read(bh_evdom* d, uint64_t* out, size_t len);
bh_status bh_evdom_write(bh_evdom* d, const uint64_t* coeffs, size_t len);
bh_status bh_evdom_into_scalars(bh_evdom* d, size_t len, bh_scalars** out);
bh_status bh_evdom_sync(bh_evdom* d);
bh_status bh_evdom_free(bh_evdom* d);

/* H block of create_proof: a, b, c hold num_constraints evaluations each (padded to m
 * internally); h_out receives m-1 Montgomery coefficients; *h_len = m-1.  Six transforms
 * instead of the reference's seven, the same h for every input: a and b take ifft +
 * coset_fft, c its ifft alone, h = icoset_fft(a*b / Z) - ifft(c) / Z (c has degree < m, so
 * icoset_fft undoes its coset_fft; icoset_fft is linear). */
bh_status bh_compute_h(bh_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                       size_t num_constraints, uint64_t* h_out, size_t* h_len);

/* ---- Parameters (groth16/mod.rs:224-477) */
/* Parameters::read format (VerifyingKey::write then u32-BE length-prefixed h, l, a, b_g1, b_g2). */
bh_status bh_params_load(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bh_params** out);
/* The same layout with every point compressed (Parameters::read of groth16/mod.rs:292-400 with
 * from_compressed in the place of from_uncompressed): the VerifyingKey's points 48 / 48 / 96 / 96 /
 * 48 / 96 bytes, the u32-BE ic length and ic at 48 B each, then h, l, a, b_g1 (48 B per point) and
 * b_g2 (96 B per point), each behind its u32-BE length.  The vectors are decoded on the device
 * (bh_srs_upload_compressed's rules), the VerifyingKey's points on the host.  Statuses are
 * bh_params_load's for the same defect: short input BH_ERR_INVALID_ENCODING; the identity refused in
 * ic and in every vector; the VerifyingKey's points always fully checked; checked adds the subgroup
 * test on the vectors (BH_ERR_NOT_IN_SUBGROUP).  The handle equals the one bh_params_load builds
 * from the same points, word for word. */
bh_status bh_params_load_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bh_params** out);
bh_status bh_params_free(bh_params* p);
/* sizes: [h, l, a, b_g1, b_g2, ic] */
bh_status bh_params_sizes(const bh_params* p, size_t out[6]);
/* ParameterSource::get_h / get_l / get_a / get_b_g1 / get_b_g2 (groth16/mod.rs:414-477): the
 * Parameters' own base vector as a bh_srs, borrowed (valid while p lives; never bh_srs_free it).
 * Multiexps over it (bh_multiexp_submit*) use the window tables bh_params_prepare built, as
 * bh_prove does: the seam then runs at the prover's per-multiexp speed. */
#define BH_VEC_H 0
#define BH_VEC_L 1
#define BH_VEC_A 2
#define BH_VEC_B_G1 3
#define BH_VEC_B_G2 4
bh_status bh_params_vector(const bh_params* p, int which, const bh_srs** out);

/* ---- prover (create_proof after synthesis, prover.rs:206-349) */
/* a,b,c: num_constraints Montgomery Fr (ProvingAssignment a/b/c incl. the input constraints);
 * assignments Montgomery; densities: bit words (a_aux: num_aux bits, b_input: num_inputs bits,
 * b_aux: num_aux bits); r, s canonical (4 LE u64).  proof_out: Proof::write, 192 B. */
bh_status bh_prove(bh_ctx* ctx, const bh_params* params, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                   size_t num_constraints, const uint64_t* input_assignment, size_t num_inputs,
                   const uint64_t* aux_assignment, size_t num_aux, const uint64_t* a_aux_density,
                   const uint64_t* b_input_density, const uint64_t* b_aux_density, const uint64_t r[4],
                   const uint64_t s[4], uint8_t proof_out[192]);
/* Same, split into an upload (witness becomes device-resident) and the proof proper. */
bh_status bh_witness_upload(bh_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                            size_t num_constraints, const uint64_t* input_assignment, size_t num_inputs,
                            const uint64_t* aux_assignment, size_t num_aux, const uint64_t* a_aux_density,
                            const uint64_t* b_input_density, const uint64_t* b_aux_density, bh_witness** out);
bh_status bh_witness_free(bh_witness* w);
/* Build now (instead of inside the first proof) the window tables that proofs of witnesses
 * shaped like w, split over nshards GPUs, will use.  Optional. */
bh_status bh_params_prepare(bh_ctx* ctx, bh_params* params, const bh_witness* w, size_t nshards);
/* The same for ONE shard: only the slices of the query vectors that shard `shard` of
 * `nshards` consumes (and, with distributed_h, its gathered share of the h vector), so that
 * a rank of a multi-GPU run holds and builds 1/nshards of the tables.  Optional. */
bh_status bh_params_prepare_shard(bh_ctx* ctx, bh_params* params, const bh_witness* w, size_t shard, size_t nshards,
                                  int distributed_h);
bh_status bh_prove_witness(bh_ctx* ctx, const bh_params* params, const bh_witness* w, const uint64_t r[4],
                           const uint64_t s[4], uint8_t proof_out[192]);

/* Throughput mode (BASELINE.json configs[4], "C5"): k independent proofs of witnesses sharing
 * one Parameters (the reference's Worker::compute fan-out, multicore.rs:33-76, r and s fixed,
 * prover.rs:158-173), every window table built once up front.  lanes (0 = default, 2): with 1
 * the proofs run back to back on ctx; with L >= 2, L host threads drive L lane contexts that
 * borrow ctx's streams (no hardware queue more) and take turns in proof order, proof i+1 being
 * enqueued as soon as proof i's device work is -- its density maps, sorts and H then run beside
 * proof i's last reduction tail and host combine.  proofs_out: k * 192 bytes, proof i ==
 * bh_prove_witness(ws[i]).  Across GPUs the batch is split by the caller (one process per GPU,
 * no collective). */
bh_status bh_prove_batch(bh_ctx* ctx, const bh_params* params, const bh_witness* const* ws, size_t k,
                         const uint64_t r[4], const uint64_t s[4], int lanes, uint8_t* proofs_out);

/* ---- multi-GPU: every multiexp sharded by scalar range (shard k of N covers
 * [k*n/N, (k+1)*n/N) of each query); partial_out = 8 uncompressed points
 * [h, l, a_inputs, a_aux, b_g1_inputs, b_g1_aux] (G1, 96 B) + [b_g2_inputs, b_g2_aux]
 * (G2, 192 B) = 960 B.  The all-gathered records are summed and assembled on the
 * host by bh_proof_from_partials (prover.rs:315-349), which needs only the
 * VerifyingKey::write bytes (bh_vk_write). */
#define BH_PARTIAL_BYTES 960
bh_status bh_shard_range(size_t n, size_t shard, size_t nshards, size_t* lo, size_t* hi);
bh_status bh_prove_witness_partial(bh_ctx* ctx, const bh_params* params, const bh_witness* w, size_t shard,
                                   size_t nshards, uint8_t partial_out[960]);
bh_status bh_vk_write(const bh_params* p, uint8_t* out, size_t cap, size_t* written);

/* ---- verification (host only, no device needed): verify_proof (verifier.rs:11-62) and the batch
 * verifier (verifier/batch.rs:95-169) over a BLS12-381 pairing.  vk: VerifyingKey::write bytes (the
 * head of Parameters::write, or bh_vk_write); proof: Proof::write bytes (192, decoded like Proof::read:
 * compressed, torsion-checked, identity rejected); public inputs: num_inputs canonical Fr, 4 LE u64
 * each, without the implicit ONE.  *valid = 1 iff the proof(s) verify; the status is non-zero only for
 * malformed data (num_inputs + 1 != ic length: BH_ERR_INVALID_ARGUMENT, the reference's
 * VerificationError::InvalidVerifyingKey).  Batch: k proofs, inputs k * num_inputs * 4 words, and the
 * caller's random nonzero scalars z (k * 4 canonical words; the reference draws them from a CryptoRng).
 * bh_verify_batch_device, further down, gives the same answers with the per-proof work on a device. */
bh_status bh_verify_proof(const uint8_t* vk, size_t vk_len, const uint8_t* proof, const uint64_t* inputs,
                          size_t num_inputs, int* valid);
bh_status bh_verify_batch(const uint8_t* vk, size_t vk_len, const uint8_t* proofs, const uint64_t* inputs,
                          size_t num_inputs, size_t k, const uint64_t* z, int* valid);
bh_status bh_proof_from_partials(const uint8_t* vk_bytes, size_t vk_len, const uint8_t* partials, size_t nshards,
                                 const uint64_t r[4], const uint64_t s[4], uint8_t proof_out[192]);

/* RCCL exchange (one communicator per rank/device; unique id shared out of band) */
typedef struct bh_comm bh_comm;
bh_status bh_comm_unique_id(uint8_t out[128]);
bh_status bh_comm_init(bh_ctx* ctx, const uint8_t id[128], int nranks, int rank, bh_comm** out);
/* all ranks' records, rank order: all_out holds nranks * BH_PARTIAL_BYTES bytes */
bh_status bh_comm_allgather_partials(bh_comm* c, const uint8_t* partial, uint8_t* all_out);
bh_status bh_comm_destroy(bh_comm* c);
/* every rank's nbytes-byte host record, rank order, into all_out (nranks * nbytes) */
bh_status bh_comm_allgather(bh_comm* c, const uint8_t* in, size_t nbytes, uint8_t* all_out);
/* max over ranks of *inout (in place, every rank); returns once every rank has called it,
 * so it is also the barrier around a timed region */
bh_status bh_comm_allreduce_max(bh_comm* c, double* inout);
/* what RCCL reports for the communicator: out = {rank count, this rank, HIP device id} */
bh_status bh_comm_info(const bh_comm* c, int out[3]);
/* This rank's partial record (rank/nranks from the communicator).  For nranks a power of two
 * in [2, 16] and m >= 2*nranks^2 the H block is distributed instead
 * of replicated: every NTT is a local m/nranks-point NTT plus one ncclSend/ncclRecv
 * all-to-all, three all-to-alls per proof, and this rank's h multiexp covers exactly the h
 * coefficients it ends with (a strided set, not the range of bh_shard_range).  Otherwise
 * identical to bh_prove_witness_partial(ctx, params, w, rank, nranks, ...). */
bh_status bh_prove_witness_partial_comm(bh_ctx* ctx, const bh_params* params, const bh_witness* w, bh_comm* comm,
                                        uint8_t partial_out[960]);
/* All nshards partial records computed on this one device by nshards virtual ranks: each a
 * context and a host thread of its own running the per-rank code of
 * bh_prove_witness_partial_comm, with device copies in place of the RCCL all-to-alls
 * (rehearsal and tests of the multi-GPU algorithm).  partials_out: nshards * BH_PARTIAL_BYTES. */
bh_status bh_prove_witness_partials_local(bh_ctx* ctx, const bh_params* params, const bh_witness* w,
                                          size_t nshards, uint8_t* partials_out);
/* The same with caller-provided ranks of one device: ctxs[k] and params[k] are rank k's context
 * and Parameters (e.g. loaded per rank and prepared with bh_params_prepare_shard, exactly as
 * the processes of a multi-GPU run hold them); the witness is shared. */
bh_status bh_prove_witness_partials_ranks(bh_ctx* const* ctxs, const bh_params* const* params, const bh_witness* w,
                                          size_t nranks, uint8_t* partials_out);
/* Rehearsal of rank `rank` of an nranks-GPU run on this one device: exactly that rank's
 * device work (its shards, the distributed H block when it applies) with each all-to-all
 * moving only the rank's own chunks; *ms = host wall time of the rank's proof.  The partial
 * sums are discarded (the data crossing ranks is missing): for timing and profiling only. */
bh_status bh_rehearse_rank(bh_ctx* ctx, const bh_params* params, const bh_witness* w, size_t rank, size_t nranks,
                           double* ms);
bh_status bh_ctx_synchronize(bh_ctx* ctx);
int bh_device_count(void);

/* ---- synthetic workload: MiMC chain (mimc_mod.rs:40-130 with R rounds, seeded constants),
 * synthesized natively (witness) and its CRS generated on the device with the classic
 * algorithm (generator.rs:310-572) from the given toxic waste (canonical u64 each). */
bh_status bh_chain_witness(bh_ctx* ctx, size_t rounds, uint64_t seed, bh_witness** out);
/* Same circuit (constants from seed), preimage (xl, xr) from preimage_seed: distinct
 * witnesses for one set of Parameters (BASELINE.json configs[4], "C5").
 * bh_chain_witness(seed) == bh_chain_witness_preimage(seed, seed + 1). */
bh_status bh_chain_witness_preimage(bh_ctx* ctx, size_t rounds, uint64_t seed, uint64_t preimage_seed,
                                    bh_witness** out);
/* The chain's ProvingAssignment on the host, in exactly the layouts bh_prove takes (the
 * drop-in path a Rust caller uses after synthesis): sizes = {constraints, inputs, aux};
 * a, b, c: constraints x 4 u64 Montgomery; inputs/aux Montgomery; density bit words. */
bh_status bh_chain_sizes(size_t rounds, size_t out[3]);
bh_status bh_chain_assignment(size_t rounds, uint64_t seed, uint64_t preimage_seed, uint64_t* a, uint64_t* b,
                              uint64_t* c, uint64_t* inputs, uint64_t* aux, uint64_t* a_aux_density,
                              uint64_t* b_input_density, uint64_t* b_aux_density);
bh_status bh_chain_params(bh_ctx* ctx, size_t rounds, uint64_t seed, uint64_t alpha, uint64_t beta, uint64_t gamma,
                          uint64_t delta, uint64_t tau, bh_params** out);

/* ---- parameter generation for any circuit: KeypairAssembly (generator.rs:44-156) resident in
 * HBM, and the classic generate_parameters (generator.rs:241-634, without the fork's MPC asserts)
 * on it. */
typedef struct bh_r1cs bh_r1cs;

/* KeypairAssembly's at_inputs .. ct_aux (generator.rs:44-60) as three column-compressed matrices,
 * one each for A, B, C, over the variables in the order [inputs (input 0 is ONE), then aux].  For
 * variable j, entries [ptr[j], ptr[j+1]) are (coeff: Montgomery Fr, 4 u64; row: constraint index,
 * u32) in the order enforce (generator.rs:113-151) appended them.  Duplicates of a (variable, row)
 * pair are allowed and add up.  ptr has num_inputs + num_aux + 1 u64 entries; row and coeff may be
 * null where a matrix has no entry.
 * num_constraints counts the circuit's own constraints only: the library appends the num_inputs
 * rows "input_i * 0 = 0" itself (generator.rs:276-282), as generate_parameters does after
 * synthesize.
 * BH_ERR_INVALID_ARGUMENT: a null pointer, num_inputs == 0, a ptr that does not start at 0 or
 * decreases, a row >= num_constraints, a coefficient >= r (all checked before anything is indexed),
 * or more than 2^32 - 1 terms in all or (2^32 - 1) / 3 variables (the device offsets are u32).
 * BH_ERR_POLY_DEGREE_TOO_LARGE: num_constraints + num_inputs exceeds the largest domain
 * (generator.rs:284-288 via domain.rs:51-60). */
bh_status bh_r1cs_create(bh_ctx* ctx, size_t num_inputs, size_t num_aux, size_t num_constraints,
                         const uint64_t* a_ptr, const uint32_t* a_row, const uint64_t* a_coeff,
                         const uint64_t* b_ptr, const uint32_t* b_row, const uint64_t* b_coeff,
                         const uint64_t* c_ptr, const uint32_t* c_row, const uint64_t* c_coeff,
                         bh_r1cs** out);
bh_status bh_r1cs_free(bh_r1cs* r);
/* out[0..7): inputs, aux, constraints including the appended input rows, terms of A (including
 * the appended ones), of B, of C, and the segment length S: the most terms one lane of the QAP
 * kernel multiplies. */
bh_status bh_r1cs_sizes(const bh_r1cs* r, size_t out[7]);
/* eval_at_tau (generator.rs:485-499) for every variable at once.  x: m Montgomery Fr, m the domain
 * size of the constraint count (the Lagrange coefficients, or any vector).  u_out, v_out, w_out
 * receive num_inputs + num_aux Montgomery Fr each: u_j = sum over column j of A of coeff * x[row],
 * likewise v (B) and w (C); an empty column gives 0. */
bh_status bh_r1cs_eval(bh_ctx* ctx, const bh_r1cs* r, const uint64_t* x, uint64_t* u_out, uint64_t* v_out,
                       uint64_t* w_out);
/* generate_parameters (generator.rs:241-634, the classic algorithm of generator.rs:310-572 and the
 * identity filter of 614-633).  Toxic waste as canonical Fr (4 LE u64 each, full width; a word
 * >= r: BH_ERR_INVALID_ARGUMENT).  gamma or delta zero: BH_ERR_UNEXPECTED_IDENTITY
 * (generator.rs:330-345).  An aux variable whose L scalar is zero: BH_ERR_UNCONSTRAINED_VARIABLE
 * (generator.rs:586-590).  An ic scalar that is zero is legal and encodes the identity.
 * The one deliberate deviation: tau = 0 or tau^m = 1 returns BH_ERR_INVALID_ARGUMENT, where the
 * reference would write identity points into the h query.
 * The result is an ordinary bh_params. */
bh_status bh_generate_parameters(bh_ctx* ctx, const bh_r1cs* r, const uint64_t alpha[4], const uint64_t beta[4],
                                 const uint64_t gamma[4], const uint64_t delta[4], const uint64_t tau[4],
                                 bh_params** out);
/* The MiMC chain's KeypairAssembly (what bh_chain_params synthesizes internally) as a bh_r1cs. */
bh_status bh_chain_r1cs(bh_ctx* ctx, size_t rounds, uint64_t seed, bh_r1cs** out);

/* ProvingAssignment (prover.rs:55-156, 187-204) evaluated on the device. r holds the circuit;
 * input_assignment: num_inputs Montgomery Fr (entry 0 is ONE), aux_assignment: num_aux Montgomery Fr.
 * a = A z, b = B z, c = C z over z = [inputs, aux], including the appended rows input_i * 0 = 0
 * (a = input_i, b = c = 0); a_aux / b_input / b_aux density bit i = variable i has at least one term
 * in that matrix, whatever its coefficient (eval calls inc before it looks at the coefficient).
 * first_unsatisfied (may be null): the least constraint index i with a_i * b_i != c_i, or SIZE_MAX.
 * The witness is returned either way; the reference's prover does not check satisfaction, this is
 * TestConstraintSystem::which_is_unsatisfied as one device pass.
 * The first call on a handle builds the row view of its matrices on the device (8 bytes per term
 * and 4 per row and row segment, kept with the handle); calls on one handle
 * run one at a time.  The result is an ordinary bh_witness, freed with bh_witness_free.
 * BH_ERR_INVALID_ARGUMENT: a null handle or pointer, r on another device than ctx, an assignment
 * word >= r. */
bh_status bh_r1cs_witness(bh_ctx* ctx, const bh_r1cs* r, const uint64_t* input_assignment,
                          const uint64_t* aux_assignment, size_t* first_unsatisfied, bh_witness** out);

/* What a resident witness holds, for tests and callers that want a/b/c back: a, b, c receive m
 * Montgomery Fr each (m = domain size; entries past num_constraints are the zero padding), inputs /
 * aux Montgomery, densities as bit words. Any pointer may be null. sizes = {num_constraints, m,
 * num_inputs, num_aux}.  Works on every witness: uploaded, chain-built or R1CS-built
 * (prover.rs:206-231 is where the reference holds the same vectors). */
bh_status bh_witness_sizes(const bh_witness* w, size_t sizes[4]);
bh_status bh_witness_read(const bh_witness* w, uint64_t* a, uint64_t* b, uint64_t* c, uint64_t* inputs,
                          uint64_t* aux, uint64_t* a_aux_density, uint64_t* b_input_density,
                          uint64_t* b_aux_density);

/* ---- per-element variable-base scalar multiplication: the primitive of a ceremony round
 * (make_new_tau_paramter, groth16/mpc.rs:677-706).  Scalars are canonical Fr (4 LE u64 each);
 * the result is a new bh_srs of the input's group and length (bh_srs_free it).
 *   BH_ERR_INVALID_ARGUMENT     a scalar >= r (or wider than nbits), mismatched lengths, a range
 *                               outside the vector
 *   BH_ERR_UNEXPECTED_IDENTITY  a result that is the identity (a zero scalar, equal points in
 *                               bh_srs_sub_range) or an identity among the inputs: a bh_srs these
 *                               calls return never holds one
 *   bh_srs_mul_each          out[i] = k_i * in[i], n == bh_srs_len(in)
 *   bh_srs_mul_each_bounded  the same for scalars below 2^nbits (1..255; leading zero windows are
 *                            skipped: a verifier's 128-bit z_i); n_scalars == bh_srs_len(in), or
 *                            1: that one scalar multiplies every element
 *   bh_srs_mul_powers        make_new_tau_paramter, mpc.rs:677-706: out[i] = (a * x^i)^(+-1) * in[i],
 *                            inverted when invert != 0 ((a x^i)^-1 = a^-1 (x^-1)^i).  The reference
 *                            forms x.pow(i) * a in u64; here it is formed in Fr, and the two agree
 *                            whenever the reference's product does not overflow.
 *   bh_srs_sub_range         out[i] = in[lo2 + i] - in[lo1 + i], i < n (mpc.rs:631-635) */
bh_status bh_srs_mul_each(bh_ctx* ctx, const bh_srs* in, const uint64_t* scalars, size_t n, bh_srs** out);
bh_status bh_srs_mul_each_bounded(bh_ctx* ctx, const bh_srs* in, const uint64_t* scalars, size_t n_scalars, int nbits,
                                  bh_srs** out);
bh_status bh_srs_mul_powers(bh_ctx* ctx, const bh_srs* in, const uint64_t a[4], const uint64_t x[4], int invert,
                            bh_srs** out);
bh_status bh_srs_sub_range(bh_ctx* ctx, const bh_srs* in, size_t lo1, size_t lo2, size_t n, bh_srs** out);

/* ---- group-valued FFT of a device point vector: EvaluationDomain<Point<G>>::fft / ifft
 * (domain.rs:81-99 with Group = Point<G>, 192-228), in G1 or G2.  Natural order in and out; omega is
 * the root the scalar EvaluationDomain of the same size uses (domain.rs:62-66); inverse != 0 uses
 * omega^-1 and scales by 1/n.  Applied to tau^i G, the inverse transform gives the Lagrange basis
 * L_i(tau) G without anyone knowing tau.  n = bh_srs_len(in) must be a power of two, 2 <= n <= 2^28:
 * anything else is BH_ERR_INVALID_ARGUMENT (a bh_srs cannot hold the identity from_coeffs pads with).
 * The one deliberate deviation: a butterfly output that is the identity, in any stage or in the
 * result, returns BH_ERR_UNEXPECTED_IDENTITY and no vector, where the reference would carry the
 * identity along (it is found on the device before the normalisation it would poison; the call
 * never returns a wrong point).  For the powers of a tau an honest player drew this happens with
 * probability at most n log n / r. */
bh_status bh_srs_fft(bh_ctx* ctx, const bh_srs* in, int inverse, bh_srs** out);

/* ---- the MPC ceremony's parameter rounds (groth16/mpc.rs), for any length and any Fr scalar where
 * the reference hard-codes length 8 and u64.  Handles belong to their context's device; toxic
 * waste is canonical Fr (a word >= r: BH_ERR_INVALID_ARGUMENT, zero: BH_ERR_UNEXPECTED_IDENTITY).
 *
 * Round one, "common" parameters (mpc.rs:362-414, 708-862):
 *   bh_mpc_common           CommonParamterInStorage (mpc.rs:398-414): alpha_g1/g2, beta_g1/g2 and
 *                           tau, alpha_mul_tau, beta_mul_tau (g1, g2 each) as device vectors of one length
 *   bh_mpc_common_contrib   CommonParamter (mpc.rs:362-373): g1_result, g2_result, g1_mine, g2_mine
 *                           for alpha, beta and every element of the three vector pairs
 *   bh_mpc_common_initial     initial_common_paramters         mpc.rs:708-728
 *   bh_mpc_common_contribute  mpc_common_paramters_generator   mpc.rs:730-785
 *   bh_mpc_common_verify      verify_common_paramter           mpc.rs:806-862.  z: len canonical
 *                             nonzero scalars drawn at random by the caller (as bh_verify_batch's;
 *                             128-bit ones suffice).  *valid = 1 and *next = the contribution's
 *                             to_storage_format() (mpc.rs:381-394) when it verifies; else 0 and NULL,
 *                             where the reference asserts.  The reference's per-element checks
 *                             (verify_new_paramter, mpc.rs:787-804) run batched: per vector pair one
 *                             multiexp of the results in each group, z_i * old_i on the device, len + 1
 *                             Miller loops and one final exponentiation on the host; every contribution
 *                             the reference accepts is accepted, one it rejects is accepted with
 *                             probability about 2^-120.  Like the reference, whose
 *                             check of the tau list is commented out (mpc.rs:831-840), it checks alpha,
 *                             beta, alpha_mul_tau, beta_mul_tau and the lengths.  It does not show that
 *                             either storage is a power sequence: run bh_mpc_common_check on a storage
 *                             of unknown origin first.
 *   bh_mpc_common_h_basis     the matrixed_h part of matrix (mpc.rs:631-635): tau[n + i] - tau[i],
 *                             i < n, in both groups; 2n > len: BH_ERR_INVALID_ARGUMENT.  The rest of
 *                             matrix is bh_mpc_common_matrix, further down.
 *   bh_mpc_common_vector / _point, bh_mpc_common_contrib_vector / _point: borrowed views (valid while
 *                             the handle lives; never bh_srs_free them) and uncompressed bytes
 *   bh_mpc_common_write / _read, bh_mpc_common_contrib_write / _read: the reference keeps these structs
 *                             in memory only; the bytes follow Parameters::write's conventions
 *                             (mod.rs:224-290).  Storage: u32-BE len, then the fields in declaration
 *                             order, G1 points uncompressed (96 B), G2 (192 B).  Contribution: the
 *                             ParameterPairs of alpha and beta (g1_result, g2_result, g1_mine, g2_mine),
 *                             then each TauParameterPair as u32-BE len and its ParameterPairs.  out ==
 *                             NULL queries the size.  checked: the on-curve and subgroup checks of
 *                             bh_params_load; the identity is refused either way.
 *   bh_mpc_common_write_compressed / _read_compressed, bh_mpc_common_contrib_write_compressed /
 *   _read_compressed:         the same layouts with every point compressed (48 B G1, 96 B G2), the
 *                             form to ship: a storage is 4 + 288 + 432 len bytes, a contribution
 *                             576 + 3 (4 + 288 len).  Arguments as the uncompressed functions.  The
 *                             vectors are coded on the device (bh_srs_upload_compressed's rules), the
 *                             handful of single points on the host.  Reading always checks flags,
 *                             range and squareness (BH_ERR_INVALID_ENCODING); checked adds the subgroup
 *                             test (BH_ERR_NOT_IN_SUBGROUP).  The identity is refused
 *                             (BH_ERR_INVALID_ENCODING); short input: BH_ERR_UNEXPECTED_EOF; trailing
 *                             bytes: BH_ERR_INVALID_ENCODING.  read_compressed then write gives the
 *                             bytes write gave before write_compressed.
 * Round two, "uncommon" parameters (mpc.rs:891-1131): UnCommonParamterInStorage (gamma_g1/g2,
 * delta_g1/g2, kin, kout, h) and UnCommonParamter (delta, gamma, ic, l, h).
 *   bh_mpc_uncommon_initial     initial_uncommon_paramters (mpc.rs:993-1015) from the six vectors of
 *                               CommonParamterMatrix (copied); a pair's lengths must agree
 *   bh_mpc_uncommon_contribute  mpc_uncommon_paramters_generator (mpc.rs:1017-1063): kin by 1/gamma,
 *                               kout and h by 1/delta
 *   bh_mpc_uncommon_verify      verify_uncommon_paramter (mpc.rs:1065-1131).  matrix: the handle
 *                               bh_mpc_uncommon_initial returned (it holds CommonParamterMatrix);
 *                               z: z_len >= the longest vector's length.  The per-element checks share
 *                               a G2 element on each side and collapse to
 *                               e(sum z_i new_i, gamma_or_delta_g2) == e(sum z_i matrix_i, G2).
 *   bytes: the four points, then each vector behind its own u32-BE length; the contribution as in
 *   round one with the ParameterPairs in the order delta, gamma.  bh_mpc_uncommon_write_compressed /
 *   _read_compressed and bh_mpc_uncommon_contrib_write_compressed / _read_compressed: the same with
 *   every point compressed, as in round one; a pair's vectors of different lengths:
 *   BH_ERR_INVALID_ENCODING. */
typedef struct bh_mpc_common bh_mpc_common;
typedef struct bh_mpc_common_contrib bh_mpc_common_contrib;
typedef struct bh_mpc_uncommon bh_mpc_uncommon;
typedef struct bh_mpc_uncommon_contrib bh_mpc_uncommon_contrib;
/* vectors of a storage / contribution (_vector's `which`) */
#define BH_MPC_TAU_G1 0
#define BH_MPC_TAU_G2 1
#define BH_MPC_ALPHA_TAU_G1 2
#define BH_MPC_ALPHA_TAU_G2 3
#define BH_MPC_BETA_TAU_G1 4
#define BH_MPC_BETA_TAU_G2 5
#define BH_MPC_KIN_G1 0
#define BH_MPC_KIN_G2 1
#define BH_MPC_KOUT_G1 2
#define BH_MPC_KOUT_G2 3
#define BH_MPC_H_G1 4
#define BH_MPC_H_G2 5
/* points of a storage (_point's `which`): common alpha_g1, alpha_g2, beta_g1, beta_g2; uncommon
 * gamma_g1, gamma_g2, delta_g1, delta_g2.  Of a contribution: 4 * pair + {0 g1_result, 1 g2_result,
 * 2 g1_mine, 3 g2_mine}, pair 0 = alpha / gamma, 1 = beta / delta.  Even: 96 B, odd: 192 B. */
bh_status bh_mpc_common_initial(bh_ctx* ctx, size_t len, bh_mpc_common** out);
bh_status bh_mpc_common_contribute(bh_ctx* ctx, const bh_mpc_common* storage, const uint64_t alpha[4],
                                   const uint64_t beta[4], const uint64_t tau[4], bh_mpc_common_contrib** out);
bh_status bh_mpc_common_verify(bh_ctx* ctx, const bh_mpc_common* storage, const bh_mpc_common_contrib* contrib,
                               const uint64_t* z, int* valid, bh_mpc_common** next);
/* ---- the structure check of a round-one storage (no counterpart in the reference; DESIGN.md
 * section 16).  bh_mpc_common_verify ties a contribution's alpha_mul_tau and beta_mul_tau lists to
 * the storage element by element and never looks at the tau lists, and bh_mpc_common_matrix
 * transforms whatever it is given; neither shows that a storage is a power sequence.  A storage of
 * length len is WELL FORMED iff scalars tau, alpha, beta exist with tau_g1[i] = tau^i G1,
 * tau_g2[i] = tau^i G2, alpha_mul_tau_g1/g2[i] = alpha tau^i G1/G2, the same for beta, and
 * alpha_g1/g2 = alpha G1/G2, beta_g1/g2 = beta G1/G2.  bh_mpc_common_initial is, and so is every
 * storage reached from it through bh_mpc_common_contribute.
 *   bh_mpc_common_check   rho: ONE canonical scalar the caller draws at random (rho >= r or zero:
 *                         BH_ERR_INVALID_ARGUMENT); the weights are w_i = rho^i, written on the
 *                         device.  With S(V) = sum_{i < len} w_i V_i, L = sum_{i < len-1} w_i tau_g1[i]
 *                         and R = sum_{i < len-1} w_i tau_g1[i+1], bit k of *failed (may be NULL) is
 *                         set iff equation k fails, and *valid = (mask == 0):
 *                           BH_MPC_CHECK_FIRST      tau_g1[0] == G1 and tau_g2[0] == G2 (bytes)
 *                           BH_MPC_CHECK_ALPHA      e(alpha_g1, G2) == e(G1, alpha_g2)
 *                           BH_MPC_CHECK_BETA       e(beta_g1, G2) == e(G1, beta_g2)
 *                           BH_MPC_CHECK_POWERS     e(R, G2) == e(L, tau_g2[1])
 *                           BH_MPC_CHECK_TAU_G2     e(S(tau_g1), G2) == e(G1, S(tau_g2))
 *                           BH_MPC_CHECK_ALPHA_TAU  e(S(alpha_mul_tau_g1), G2) == e(S(tau_g1), alpha_g2)
 *                           BH_MPC_CHECK_ALPHA_TAU_G2   ... == e(G1, S(alpha_mul_tau_g2))
 *                           BH_MPC_CHECK_BETA_TAU, BH_MPC_CHECK_BETA_TAU_G2   the same two for beta
 *                         Every equation is evaluated (no early exit); a sum that is the identity
 *                         pairs to one.  FIRST is vacuous for len = 0 and POWERS for len < 2; len = 0
 *                         evaluates ALPHA and BETA only.  A well-formed storage always passes; a
 *                         malformed one passes an equation it violates with probability at most
 *                         len / r over rho (below 2^-226 for len <= 2^28).  Cost: eight multiexps of
 *                         length len (five in G1, three in G2) and nine pairing equations on the
 *                         host's pool, whatever len is.
 *   bh_mpc_common_verify_structure   verifies a contribution with O(1) pairings.  PRECONDITION:
 *                         storage is well formed -- it is the initial one, or bh_mpc_common_check
 *                         accepted it, or it came out of this function.  Accepts iff
 *                           BH_MPC_CHECK_LENGTHS     all twelve vectors of contrib have storage's length
 *                                                    (if not, this bit alone is set and nothing else runs)
 *                           BH_MPC_CHECK_ALPHA_RATIO e(R1, G2) == e(O1, M2), the first equation of
 *                                                    verify_new_paramter (mpc.rs:787-804), O1 = storage's
 *                                                    alpha_g1, R1 = the result, M2 = the player's g2_mine
 *                           BH_MPC_CHECK_BETA_RATIO  the same for beta
 *                           BH_MPC_CHECK_TAU_RATIO   the same for element 1 of the tau pair: O1 = storage's
 *                                                    tau_g1[1], R1 = the result's, M2 = mine tau_g2[1]
 *                                                    (vacuous for len < 2)
 *                           bits 0-8                 bh_mpc_common_check of contrib's to_storage_format()
 *                         On acceptance *valid = 1 and *next is that storage, byte-identical under
 *                         bh_mpc_common_write to what bh_mpc_common_verify returns; else 0 and NULL.
 *                         It accepts everything bh_mpc_common_contribute makes from a well-formed
 *                         storage and refuses tau lists bh_mpc_common_verify lets through.  The
 *                         "mine" lists are NOT read beyond the three g2_mine above: the per-element
 *                         proofs they carry are implied by the two storages being power sequences.
 *   bh_mpc_last_check_ms  wall time (ms) of this thread's last check (either function): [0] the
 *                         weights and the multiexps, [1] the pairings */
#define BH_MPC_CHECK_FIRST (1u << 0)
#define BH_MPC_CHECK_ALPHA (1u << 1)
#define BH_MPC_CHECK_BETA (1u << 2)
#define BH_MPC_CHECK_POWERS (1u << 3)
#define BH_MPC_CHECK_TAU_G2 (1u << 4)
#define BH_MPC_CHECK_ALPHA_TAU (1u << 5)
#define BH_MPC_CHECK_ALPHA_TAU_G2 (1u << 6)
#define BH_MPC_CHECK_BETA_TAU (1u << 7)
#define BH_MPC_CHECK_BETA_TAU_G2 (1u << 8)
#define BH_MPC_CHECK_LENGTHS (1u << 9)
#define BH_MPC_CHECK_ALPHA_RATIO (1u << 10)
#define BH_MPC_CHECK_BETA_RATIO (1u << 11)
#define BH_MPC_CHECK_TAU_RATIO (1u << 12)
bh_status bh_mpc_common_check(bh_ctx* ctx, const bh_mpc_common* storage, const uint64_t rho[4], int* valid,
                              uint32_t* failed);
bh_status bh_mpc_common_verify_structure(bh_ctx* ctx, const bh_mpc_common* storage,
                                         const bh_mpc_common_contrib* contrib, const uint64_t rho[4], int* valid,
                                         uint32_t* failed, bh_mpc_common** next);
void bh_mpc_last_check_ms(double out[2]);
bh_status bh_mpc_common_h_basis(bh_ctx* ctx, const bh_mpc_common* storage, size_t n, bh_srs** h_g1, bh_srs** h_g2);
size_t bh_mpc_common_len(const bh_mpc_common* storage);
bh_status bh_mpc_common_free(bh_mpc_common* storage);
bh_status bh_mpc_common_vector(const bh_mpc_common* storage, int which, const bh_srs** out);
bh_status bh_mpc_common_point(const bh_mpc_common* storage, int which, uint8_t* out);
bh_status bh_mpc_common_write(const bh_mpc_common* storage, uint8_t* out, size_t cap, size_t* written);
bh_status bh_mpc_common_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bh_mpc_common** out);
bh_status bh_mpc_common_write_compressed(const bh_mpc_common* storage, uint8_t* out, size_t cap, size_t* written);
bh_status bh_mpc_common_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                        bh_mpc_common** out);
bh_status bh_mpc_common_contrib_free(bh_mpc_common_contrib* contrib);
bh_status bh_mpc_common_contrib_vector(const bh_mpc_common_contrib* contrib, int which, int mine, const bh_srs** out);
bh_status bh_mpc_common_contrib_point(const bh_mpc_common_contrib* contrib, int which, uint8_t* out);
bh_status bh_mpc_common_contrib_write(const bh_mpc_common_contrib* contrib, uint8_t* out, size_t cap,
                                      size_t* written);
bh_status bh_mpc_common_contrib_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                     bh_mpc_common_contrib** out);
bh_status bh_mpc_common_contrib_write_compressed(const bh_mpc_common_contrib* contrib, uint8_t* out, size_t cap,
                                                 size_t* written);
bh_status bh_mpc_common_contrib_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                                bh_mpc_common_contrib** out);
bh_status bh_mpc_uncommon_initial(bh_ctx* ctx, const bh_srs* front_g1, const bh_srs* front_g2, const bh_srs* back_g1,
                                  const bh_srs* back_g2, const bh_srs* h_g1, const bh_srs* h_g2,
                                  bh_mpc_uncommon** out);
bh_status bh_mpc_uncommon_contribute(bh_ctx* ctx, const bh_mpc_uncommon* storage, const uint64_t gamma[4],
                                     const uint64_t delta[4], bh_mpc_uncommon_contrib** out);
bh_status bh_mpc_uncommon_verify(bh_ctx* ctx, const bh_mpc_uncommon* matrix, const bh_mpc_uncommon* storage,
                                 const bh_mpc_uncommon_contrib* contrib, const uint64_t* z, size_t z_len, int* valid,
                                 bh_mpc_uncommon** next);
bh_status bh_mpc_uncommon_free(bh_mpc_uncommon* storage);
bh_status bh_mpc_uncommon_vector(const bh_mpc_uncommon* storage, int which, const bh_srs** out);
bh_status bh_mpc_uncommon_point(const bh_mpc_uncommon* storage, int which, uint8_t* out);
bh_status bh_mpc_uncommon_write(const bh_mpc_uncommon* storage, uint8_t* out, size_t cap, size_t* written);
bh_status bh_mpc_uncommon_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked, bh_mpc_uncommon** out);
bh_status bh_mpc_uncommon_write_compressed(const bh_mpc_uncommon* storage, uint8_t* out, size_t cap, size_t* written);
bh_status bh_mpc_uncommon_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                          bh_mpc_uncommon** out);
bh_status bh_mpc_uncommon_contrib_free(bh_mpc_uncommon_contrib* contrib);
bh_status bh_mpc_uncommon_contrib_vector(const bh_mpc_uncommon_contrib* contrib, int which, int mine,
                                         const bh_srs** out);
bh_status bh_mpc_uncommon_contrib_point(const bh_mpc_uncommon_contrib* contrib, int which, uint8_t* out);
bh_status bh_mpc_uncommon_contrib_write(const bh_mpc_uncommon_contrib* contrib, uint8_t* out, size_t cap,
                                        size_t* written);
bh_status bh_mpc_uncommon_contrib_read(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                       bh_mpc_uncommon_contrib** out);
bh_status bh_mpc_uncommon_contrib_write_compressed(const bh_mpc_uncommon_contrib* contrib, uint8_t* out,
                                                   size_t cap, size_t* written);
bh_status bh_mpc_uncommon_contrib_read_compressed(bh_ctx* ctx, const uint8_t* bytes, size_t len, int checked,
                                                  bh_mpc_uncommon_contrib** out);
/* ---- between the rounds: CommonParamterInStorage::matrix (mpc.rs:597-645) for ANY circuit, and
 * the Parameters of the finished ceremony (generate_parameters_mpc, generator.rs:163-237, whose a,
 * b_g1 and b_g2 the reference leaves empty).
 *   bh_mpc_common_matrix   with m the domain size of r (constraints plus the appended input rows):
 *                          the inverse bh_srs_fft of the first m elements of the storage's six
 *                          vectors, then the circuit's matrices applied to those Lagrange bases as
 *                          list_mul_matrix (mpc.rs:416-457) and eval (generator.rs:411-510) apply
 *                          them to scalars: out_j = sum over column j's terms of coeff * Lag[row].
 *                          The handle holds nine vectors (bh_mpc_matrix_vector, borrowed):
 *                            BH_MPC_KIN_G1 .. BH_MPC_H_G2   kin = beta A_j + alpha B_j + C_j of the
 *                              inputs, kout the same of the aux variables, each in G1 and G2, and
 *                              h = bh_mpc_common_h_basis(m): the six of bh_mpc_uncommon_initial
 *                            BH_MPC_MATRIX_A / _B_G1 / _B_G2   A_j(tau) G1, B_j(tau) G1, B_j(tau) G2
 *                              over [inputs, aux], identities filtered out with the order kept
 *                              (generator.rs:614-632)
 *                          kin is the INPUTS' block: the contract is generate_parameters
 *                          (generator.rs:520-572), where ic is the inputs' block over gamma and l the
 *                          aux block over delta.  The reference's matrix puts the aux block in front
 *                          and initial_uncommon_paramters makes the front kin (mpc.rs:597-612,
 *                          1008-1011); divided by gamma that is not a Groth16 ic.
 *                          BH_ERR_INVALID_ARGUMENT: a null handle, a handle of another device,
 *                          bh_mpc_common_len(storage) < 2m, m < 2, tau_g1[0] not the generator (the
 *                          reference asserts it, mpc.rs:632).  BH_ERR_UNCONSTRAINED_VARIABLE: an aux
 *                          variable whose kout is the identity (generator.rs:586-590).
 *                          BH_ERR_UNEXPECTED_IDENTITY: an identity among kin or h, or from a transform.
 *                          Beyond tau_g1[0] the vectors are taken as given: run bh_mpc_common_check
 *                          on a storage of unknown origin first.
 *   bh_mpc_parameters      generator.rs:207-236 with the queries filled in: vk = alpha_g1, beta_g1,
 *                          beta_g2 of round one, gamma_g2, delta_g1, delta_g2 of round two, ic = round
 *                          two's kin_g1; l = kout_g1; h = the first m - 1 of h_g1; a, b_g1, b_g2 from
 *                          the matrix.  Round-two vectors whose lengths are not the matrix' (inputs,
 *                          aux, m): BH_ERR_INVALID_ARGUMENT.  The result is an ordinary bh_params. */
typedef struct bh_mpc_matrix bh_mpc_matrix;
#define BH_MPC_MATRIX_A 6
#define BH_MPC_MATRIX_B_G1 7
#define BH_MPC_MATRIX_B_G2 8
bh_status bh_mpc_common_matrix(bh_ctx* ctx, const bh_mpc_common* storage, const bh_r1cs* r, bh_mpc_matrix** out);
bh_status bh_mpc_matrix_vector(const bh_mpc_matrix* matrix, int which, const bh_srs** out);
bh_status bh_mpc_matrix_free(bh_mpc_matrix* matrix);
bh_status bh_mpc_parameters(bh_ctx* ctx, const bh_mpc_common* round1, const bh_mpc_matrix* matrix,
                            const bh_mpc_uncommon* round2, bh_params** out);
/* wall time (ms) of the parts of this thread's last bh_mpc_common_matrix: [0] the six inverse
 * transforms, [1] the matrix product, [2] the h basis (every part synchronises) */
void bh_mpc_last_matrix_ms(double out[3]);

/* ---- Parameters checked against a circuit and a round-one storage (no counterpart in the
 * reference).  bh_params_load(checked = 1) shows that the points of received
 * Parameters are in the subgroup, nothing more; the only other way to know that they belong to THIS
 * circuit and THIS power sequence is to rebuild them (bh_mpc_common_matrix and every round-two
 * contribution) and compare bytes.  With tau, alpha, beta the scalars of a well-formed storage S
 * (above), n = inputs + aux variables and m the domain size of r, Parameters P are VALID FOR (r, S)
 * iff gamma, delta != 0 exist such that P is byte for byte what bh_generate_parameters returns for
 * r, alpha, beta, gamma, delta, tau (generator.rs:520-572, 614-633) -- which is also what
 * bh_mpc_parameters returns after any round two.
 *   bh_params_check   PRECONDITIONS: storage is well formed -- the initial one, or one accepted by
 *                     bh_mpc_common_check / bh_mpc_common_verify_structure; p was loaded checked or
 *                     made by the library.  rho, sigma: TWO canonical scalars the caller draws
 *                     independently at random.  BH_ERR_INVALID_ARGUMENT: a null handle or a handle on
 *                     another device; rho or sigma zero or >= r; bh_mpc_common_len(storage) < 2m;
 *                     m < 2.  With x_i = sigma^i, i < m, and u, v, w = bh_r1cs_eval at x, column j of
 *                     A is PRESENT iff u_j != 0 and column j of B iff v_j != 0 (a column whose terms
 *                     cancel has u_j = 0 for every sigma; the generator filters it too).  The
 *                     weights are w_j = rho^j over [inputs, aux]; w_in = w on the inputs and zero
 *                     elsewhere, w_aux = w - w_in, w^A / w^B = w compacted to the present columns of
 *                     A / B with the order kept.  For a matrix M and weights z, c_M(z) is the inverse
 *                     NTT (size m, with the 1/m) of the row vector M z, the appended input rows
 *                     included: bh_r1cs_witness's a, b, c for the assignment z, so that
 *                     sum_k c_M(z)_k tau^k = sum_j z_j M_j(tau).  T, AT, BT, T2 are the storage's
 *                     tau_g1, alpha_mul_tau_g1, beta_mul_tau_g1, tau_g2; <V, s> is a multiexp;
 *                     K(z) = <BT, c_A(z)> + <AT, c_B(z)> + <T, c_C(z)> over the first m elements.
 *                     Bit k of *failed (may be NULL) is set iff equation k fails, *valid = (mask == 0):
 *                       BH_PARAMS_CHECK_SIZES  ic = inputs, l = aux, h = m - 1, a = the present columns
 *                                              of A, b_g1 = b_g2 = those of B (if not, this bit alone
 *                                              is set and nothing else runs)
 *                       BH_PARAMS_CHECK_ALPHA  vk.alpha_g1 == the storage's alpha_g1 (bytes)
 *                       BH_PARAMS_CHECK_BETA   vk.beta_g1, vk.beta_g2 == the storage's (bytes)
 *                       BH_PARAMS_CHECK_DELTA  e(delta_g1, G2) == e(G1, delta_g2), and neither
 *                                              gamma_g2 nor delta_g2 is the identity
 *                       BH_PARAMS_CHECK_A      <a, w^A> == <T, c_A(w)>  (equal points, no pairing)
 *                       BH_PARAMS_CHECK_B_G1   <b_g1, w^B> == <T, c_B(w)>
 *                       BH_PARAMS_CHECK_B_G2   <b_g2, w^B> == <T2, c_B(w)>
 *                       BH_PARAMS_CHECK_L      e(<l, w_aux>, delta_g2) == e(K(w_aux), G2),
 *                                              K(w_aux) computed as K(w) - K(w_in)
 *                       BH_PARAMS_CHECK_IC     e(<ic, w_in>, gamma_g2) == e(K(w_in), G2)
 *                       BH_PARAMS_CHECK_H      e(sum_{i < m-1} rho^i h_i, delta_g2)
 *                                                == e(sum_{i < m-1} rho^i (T[i + m] - T[i]), G2),
 *                                              the right side one multiexp of length 2m, signed weights
 *                     Every equation is evaluated (no early exit); a sum that is the identity pairs
 *                     to one.  Valid Parameters pass unless sigma is a root of a present column's
 *                     polynomial (probability below 2 n m / r; SIZES is then set); invalid ones pass
 *                     an equation they violate with probability below 3 n m / r over (rho, sigma),
 *                     below 2^-190 for every size bh_r1cs_create accepts.  Cost: two row products, six scalar inverse
 *                     NTTs of size m, sixteen multiexps (fourteen in G1, two in G2: nine of
 *                     length m, one of 2m, six over the Parameters' own vectors) and four
 *                     pairing equations on the host's pool; no group FFT, and no scalar vector
 *                     crosses the host link.
 *   bh_params_last_check_ms   wall time (ms) of this thread's last bh_params_check: [0] the scalar
 *                     side (powers, evaluation, row products, NTTs), [1] the multiexps, [2] the
 *                     byte comparisons and pairings */
#define BH_PARAMS_CHECK_SIZES (1u << 0)
#define BH_PARAMS_CHECK_ALPHA (1u << 1)
#define BH_PARAMS_CHECK_BETA (1u << 2)
#define BH_PARAMS_CHECK_DELTA (1u << 3)
#define BH_PARAMS_CHECK_A (1u << 4)
#define BH_PARAMS_CHECK_B_G1 (1u << 5)
#define BH_PARAMS_CHECK_B_G2 (1u << 6)
#define BH_PARAMS_CHECK_L (1u << 7)
#define BH_PARAMS_CHECK_IC (1u << 8)
#define BH_PARAMS_CHECK_H (1u << 9)
bh_status bh_params_check(bh_ctx* ctx, const bh_params* p, const bh_r1cs* r, const bh_mpc_common* storage,
                          const uint64_t rho[4], const uint64_t sigma[4], int* valid, uint32_t* failed);
void bh_params_last_check_ms(double out[3]);

/* wall time (ms) the per-element Miller loops took in this thread's last bh_mpc_common_verify, on
 * whichever path ran them: the device product below (the default), or the host's pool threads
 * (with BH_MPC_HOST_MILLER=1 in the environment, a diagnostic mode, and for a vector pair whose
 * device product reported BH_ERR_PAIRING_DEGENERATE, so that the verdict is the host's) */
double bh_mpc_last_miller_ms(void);
/* how many vector pairs of that verification ran their Miller loops on the device */
int bh_mpc_last_miller_device(void);

/* ---- pairing products over device vectors.
 * bh_miller_product: prod_{i < n} f(g1[off1 + i], g2[off2 + i]) before the final exponentiation --
 * multi_miller_loop of the bls12_381 crate as verifier.rs and mpc.rs:787-804 use it -- computed on
 * the device for a G1 and a G2 vector of the context's device.  Conventions as the library's host
 * verifier: Fp12 = Fp2[w]/(w^6 - xi), xi = 1 + u; affine line functions scaled by w^3; the loop over
 * |x| (the sign of x only inverts every value, so a product-equals-one check is unaffected); a pair
 * with an identity on either side contributes one.  out: the twelve Fp coefficients c[0].c0,
 * c[0].c1, ..., c[5].c1 of sum_k c[k] w^k, 48 bytes big-endian canonical each (the byte convention
 * of point coordinates); n = 0 gives one.  BH_ERR_INVALID_ARGUMENT: a null pointer, g1 not a G1 or
 * g2 not a G2 vector, a range past a vector's end.  BH_ERR_PAIRING_DEGENERATE: a step met a zero
 * denominator, which no point of the order-r subgroup causes; out is then not written.
 * bh_final_exponentiation: out = f^((p^12 - 1) / r) in the same encoding (host only, no context);
 * BH_ERR_INVALID_ENCODING for a coefficient >= p. */
bh_status bh_miller_product(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2, size_t n,
                            uint8_t out[576]);
bh_status bh_final_exponentiation(const uint8_t f[576], uint8_t out[576]);
/* bh_final_exponentiation of n values on the context's device: f and out hold n x 576 bytes in the
 * encoding above, and out[i] equals bh_final_exponentiation(f[i]) byte for byte for every canonical
 * input (zero gives zero).  The verifier's final step (verifier.rs:23-62 compares one such value
 * per proof), computed with the exponent (p^12 - 1) / r split into its easy part and a short
 * addition chain for the hard part instead of the host's square-and-multiply ladder.
 * BH_ERR_INVALID_ENCODING: a coefficient >= p in any value; nothing is written then.  n = 0: BH_OK.
 * out may be f. */
bh_status bh_final_exponentiation_batch(bh_ctx* ctx, const uint8_t* f, size_t n, uint8_t* out);

/* ---- vectors of target-group values (the fork's gt_bytes.rs / gt_utils.rs: pairing(g1, g2),
 * gt + gt, gt * Scalar, -gt as 576-byte strings).  A bh_gt is a vector of n Gt values resident on
 * the context's device, in the convention of the bls12_381 crate: with e0(P, Q) the final
 * exponentiation of the Miller value above, a bh_gt element is conj(e0(P, Q))^3.
 * gt_format (gt_bytes.rs:32-74), the byte form of every entry point below: the six Fp2 coefficients
 * of w^5, w^3, w^1, w^4, w^2, w^0 in that order, each c1 then c0, each Fp 48 bytes big-endian
 * canonical.
 * Common rules: a null pointer, a handle of another device than ctx's or a range past a vector's end
 * is BH_ERR_INVALID_ARGUMENT; n = 0 is BH_OK and gives an empty vector; on any error no handle is
 * returned.  Every returned bh_gt is freed by the caller.
 *   pairing      out[i] = pairing(g1[off1 + i], g2[off2 + i]) (gt_bytes.rs:210), i < n; a pair with
 *                an identity on either side gives one.  Ranges, groups and
 *                BH_ERR_PAIRING_DEGENERATE as the Miller product above; no vector is made then.
 *   from_miller  f: n x 576 bytes in the Miller product's encoding; out[i] =
 *                conj(f_i^((p^12 - 1) / r))^3, so that products built with the calls above become Gt
 *                values.  A coefficient >= p: BH_ERR_INVALID_ENCODING.
 *   upload       n x 576 bytes of gt_format.  A coefficient >= p is always
 *                BH_ERR_INVALID_ENCODING.  checked adds membership: frob^4(f) f = frob^2(f), then
 *                f^r = 1; a failure is BH_ERR_NOT_IN_SUBGROUP.  Unchecked values outside Gt give
 *                unspecified results in the calls below, never a fault.
 *   read         elements first .. first + n as gt_format bytes.
 *   add          elementwise gt + gt, the Fp12 product; the lengths must be equal.
 *   neg          -gt, the conjugate.
 *   mul_each     gt * Scalar with canonical Fr scalars (4 little-endian u64 each); n_scalars is the
 *                length of a, or 1 for one scalar applied to every element.  A scalar >= r:
 *                BH_ERR_INVALID_ARGUMENT.  A zero scalar gives one.
 *   sum          the sum of all elements as gt_format bytes; none gives one.
 *   multiexp     sum_i scalars[i] a[i] (one scalar per element): mul_each, then sum. */
typedef struct bh_gt bh_gt;
bh_status bh_gt_pairing(bh_ctx* ctx, const bh_srs* g1, size_t off1, const bh_srs* g2, size_t off2, size_t n,
                        bh_gt** out);
bh_status bh_gt_from_miller(bh_ctx* ctx, const uint8_t* f, size_t n, bh_gt** out);
bh_status bh_gt_upload(bh_ctx* ctx, const uint8_t* bytes, size_t n, int checked, bh_gt** out);
bh_status bh_gt_read(const bh_gt* gt, size_t first, size_t n, uint8_t* out);
size_t bh_gt_len(const bh_gt* gt);
bh_status bh_gt_free(bh_gt* gt);
bh_status bh_gt_add(bh_ctx* ctx, const bh_gt* a, const bh_gt* b, bh_gt** out);
bh_status bh_gt_neg(bh_ctx* ctx, const bh_gt* a, bh_gt** out);
bh_status bh_gt_mul_each(bh_ctx* ctx, const bh_gt* a, const uint64_t* scalars, size_t n_scalars, bh_gt** out);
bh_status bh_gt_sum(bh_ctx* ctx, const bh_gt* a, uint8_t out[576]);
bh_status bh_gt_multiexp(bh_ctx* ctx, const bh_gt* a, const uint64_t* scalars, uint8_t out[576]);

/* ---- batch verification on the device (verifier/batch.rs:95-169).
 * bh_verify_batch_device: for every input the status and *valid of bh_verify_batch, with the
 * per-proof work on the context's device: Proof::read of the k proofs (bh_proofs_decode's kernels),
 * z_i A_i, sum z_i C_i and the product of the k Miller values f(z_i A_i, B_i).  The Fr sums over the
 * public inputs, the three remaining Miller loops and the one final exponentiation stay on the host.
 * Where the reference pairs z A with -B, neither is negated here: the three accumulated G1 points
 * are, which inverts the whole product and leaves the verdict unchanged.  Errors in the host's
 * order: the verifying key and the input count; then, walking j = 0 .. k-1, the first of z_j (>= r
 * or zero: BH_ERR_INVALID_ARGUMENT), proof j (A, B, C) and proof j's inputs (>= r).  k = 0 is valid.
 * There is no size switch inside: the caller chooses between the two functions.  Should the device
 * product report BH_ERR_PAIRING_DEGENERATE (no subgroup-checked B causes that), the whole batch runs
 * through bh_verify_batch and its answer is returned. */
bh_status bh_verify_batch_device(bh_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint8_t* proofs,
                                 const uint64_t* inputs, size_t num_inputs, size_t k, const uint64_t* z,
                                 int* valid);
/* ---- every proof of a list on the device (verifier.rs:23-62 per item).  The batch verifier above
 * answers for the whole batch and loses "the ability to easily pinpoint failing proofs"
 * (verifier/batch.rs:3-8); the reference gives every item Item::verify_single "for implementing
 * fallback logic when batch verification fails" (batch.rs:54-60).  This is that fallback for all k
 * items at once: for every j < k, status[j] and valid[j] are what
 *   bh_verify_proof(vk, vk_len, proofs + 192 j, inputs + 4 j num_inputs, num_inputs, &v)
 * returns and sets -- proof j's decode status first, in the order A, B, C; then an input >= r:
 * BH_ERR_INVALID_ARGUMENT; valid[j] = 0 whenever status[j] is non-zero -- and one malformed or
 * invalid proof does not touch the others.  The return value reports only what all items share: a
 * null pointer, the verifying key's own status, num_inputs + 1 != ic length
 * (BH_ERR_INVALID_ARGUMENT) and failures of the run; k = 0 is BH_OK.  status: k words, valid: k
 * bytes.  On the device: Proof::read, acc_j = ic_0 + sum_i x_ji ic_i, per proof the Miller loops
 * f(A_j, B_j) f(-acc_j, gamma) f(-C_j, delta) (G1 points negated where bh_verify_proof negates
 * gamma and delta: the pairing values are the same), the product by f(-alpha, beta), which the
 * host computes once per call, the final exponentiation (bh_final_exponentiation_batch's kernels)
 * and the comparison with one; k words come back.  There is no size switch inside: the caller
 * chooses between this and a loop over bh_verify_proof.  Should a Miller step report
 * BH_ERR_PAIRING_DEGENERATE (no subgroup-checked B, gamma or delta causes that), every item is
 * answered by bh_verify_proof. */
bh_status bh_verify_each_device(bh_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint8_t* proofs,
                                const uint64_t* inputs, size_t num_inputs, size_t k, uint32_t* status,
                                uint8_t* valid);
/* Proof::read of k proofs (192 bytes each: compressed A, B, C) on the device, each point as the host
 * verifier decodes it: compression flag clear, infinity flag set, a coordinate >= p (the three flag
 * bits are masked on a point's first 48 bytes only), x^3 + b not a square: BH_ERR_INVALID_ENCODING;
 * [r]P != O: BH_ERR_NOT_IN_SUBGROUP.  status[j] (k words, may be NULL) = BH_OK or the error of
 * proof j's first failing point in the order A, B, C.  All zero: *a, *b, *c are new bh_srs of k
 * points (G1, G2, G1; B as encoded, not negated), to be freed by the caller.  Otherwise they are
 * NULL and the call returns the status of the lowest failing j.  k = 0: BH_OK and three empty
 * vectors. */
bh_status bh_proofs_decode(bh_ctx* ctx, const uint8_t* proofs, size_t k, uint32_t* status, bh_srs** a, bh_srs** b,
                           bh_srs** c);

/* Parameters::write of device-resident params (groth16/mod.rs:260-290); the vectors are encoded on
 * the device.  out == NULL: *written = the size, from the lengths alone. */
bh_status bh_params_write(const bh_params* p, uint8_t* out, size_t cap, size_t* written);
/* The same layout with every point compressed (Parameters::write with into_compressed in the place
 * of into_uncompressed, groth16/mod.rs:260-290): what bh_params_load_compressed reads. */
bh_status bh_params_write_compressed(const bh_params* p, uint8_t* out, size_t cap, size_t* written);

/* ---- profile of the last bh_prove_witness[_partial] (device events):
 * [0] host wall ms, [1] H pipeline ms, [2] G1 accumulation ms (sum over launches),
 * [3] G1 accumulation launches, [4] G1 (base, scalar) pairs, [5] G2 accumulation ms,
 * [6] G2 launches, [7] G2 pairs, [8] G1 mixed additions, [9] G2 mixed additions */
bh_status bh_last_timings(const bh_ctx* ctx, double out[10]);
/* bh_last_timings' fields followed by [10] large multiexps that used a window table,
 * [11] large multiexps (those a table would serve), [12] bytes of the window tables the proof
 * read (each distinct table once: for a shard, its own slices); after a bh_prove from host
 * buffers, [13] ms from the call's start until inputs + aux had landed on the device, [14..16]
 * until a, b, c had, [17] until the H block was done; after bh_fft / bh_ifft / bh_coset_fft /
 * bh_icoset_fft, [18] upload, [19] transform, [20] download ms of the last call; after a proof,
 * [21] / [22] the wall time (ms) during which at least one G1 / G2 bucket accumulation ran (the
 * union of their launches; [2] and [5] sum the launches, which can overlap); n entries are
 * written (missing ones 0). */
bh_status bh_last_stats(const bh_ctx* ctx, double* out, size_t n);

/* ---- scratch budget (no reference counterpart: a guard the device needs).  A spilling kernel's
 * scratch is provisioned per hardware queue for the waves it can have in flight, out of one
 * device-wide amount; exceeding it aborts inside the runtime (HSA_STATUS_ERROR_OUT_OF_RESOURCES).
 * The library checks its kernels (private segment per lane x 64 x resident waves, times the
 * queues a context runs them on) against the device limit before every proof and multiexp, which
 * return BH_ERR_SCRATCH_LIMIT instead.  out[0..n): [0] device scratch limit (bytes, shared by all
 * queues; 0 unknown), [1] current per-queue threshold, [2] worst private segment (bytes/lane),
 * [3] its per-queue need at the scratch-slot bound (32 waves per CU), [4] queues counted, [5] the
 * context's total need, [6] fits (1/0), [7] kernels checked, [8] the worst kernel's per-queue need
 * at its occupancy, [9] live contexts on the device (refreshed on every call); worst_kernel
 * (optional, cap bytes): that kernel's name.  [6] decides for ONE context's queues: a caller that
 * runs several contexts' proofs at once on one device must budget [5] x [9] itself (batch lanes
 * borrow their primary's streams; the one-device rehearsal's ranks prove one after another). */
bh_status bh_scratch_report(bh_ctx* ctx, uint64_t* out, size_t n, char* worst_kernel, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* BELLMAN_HIP_H */
