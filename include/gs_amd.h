/* gs_amd.h -- C ABI of the MI355X-native Groth-Sahai prove/verify engine.
 *
 * Drop-in boundary for the hot path of jdwhite48/groth-sahai-rs.  The reference
 * has no FFI layer; these entry points are what a Rust `extern "C"` shim
 * implementing its public traits would bind (INTEGRATION.md shows the shim):
 *
 *   gs_commit_*            <- src/prover/commit.rs:59-256  (commit_G1, batch_commit_G1, ... scalar_to_B2)
 *   gs_prove_batch         <- src/prover/prove.rs:92-171,195-274,298-379,409-488  (Provable::prove), and with
 *                             xcoms/ycoms != NULL src/prover/prove.rs:72-90,175-193,278-296,383-408 (commit_and_prove)
 *   gs_verify_batch        <- src/verifier.rs:23-157       (Verifiable::verify, exact semantics, bool per equation)
 *   gs_verify_batch_rlc    <- (new) batched pairing-product check, one final exponentiation per batch
 *   gs_verify_batch_rlc_locate <- (new) the same check with the product tree kept and descended: which proofs are bad
 *   gs_rerandomize_batch   <- (new) rerandomization of commitments and proofs without the witness (the same
 *                             algebra as src/prover/prove.rs:92-171,195-274,298-379,409-488 applied to fresh randomness)
 *   gs_simulate_batch      <- (new) commitments and proofs WITHOUT a witness from the trapdoor of the hiding CRS, the
 *                             simulation key that src/generator.rs:65-77 prepares and nothing in the reference uses
 *   gs_eval_batch / gs_check_witness_batch <- (new) the left-hand sides of src/statement.rs:17-21 at a witness: an
 *                             equation's target, and whether a witness satisfies it (tests/prover.rs:50-52,87-90,125-128,
 *                             160-162 write the same sums by hand with arkworks)
 *   gs_mat_left_mul_com1/2 <- src/data_structures.rs:696-742 (Mat::left_mul on Matrix<Com1/Com2>)
 *   gs_pairing_sum         <- src/data_structures.rs:494-502 (ComT::pairing_sum)
 *   gs_set_crs             <- consumes src/generator.rs:35-42 (struct CRS)
 *
 * DATA LAYOUT (arkworks' in-memory limbs; all little-endian):
 *   Fq  = NQ u64 limbs of a*2^(64 NQ) mod p   (BLS12-381: NQ=6, 48 B; BN254: NQ=4, 32 B)
 *   Fr  = 4 u64 limbs of a*2^256 mod r        (32 B, Montgomery)
 *   G1  = x || y                (identity = all-zero bytes)
 *   G2  = x.c0 || x.c1 || y.c0 || y.c1        (identity = all-zero bytes)
 *   Com1 = G1 || G1,  Com2 = G2 || G2
 *   GT  = 12 Fq, order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1
 *   CRS = u[0],u[1] (Com1) || v[0],v[1] (Com2) || g1 || g2 || gt
 * Batches are arrays-of-structs, equation-major, row-major inside an equation
 * (Gamma[N][m][n], R[N][m][kx], S[N][n][ky], T[N][ky][kx]).
 *
 * Equation types and shapes (kx = columns of R = #pi, ky = columns of S = #theta):
 *   GS_PPE    : X in G1^m, Y in G2^n, A in G1^n, B in G2^m, target GT,  kx=2, ky=2
 *   GS_MSMEG1 : X in G1^m, y in Fr^n, A in G1^n, b in Fr^m, target G1,  kx=2, ky=1
 *   GS_MSMEG2 : x in Fr^m, Y in G2^n, a in Fr^n, B in G2^m, target G2,  kx=1, ky=2
 *   GS_QUAD   : x in Fr^m, y in Fr^n, a in Fr^n, b in Fr^m, target Fr,  kx=1, ky=1
 *
 * Randomness (R, S, T) is an input of every entry point that computes what the
 * reference computes: the shim draws it from the caller's Rng in the reference's
 * order (R row-major, then S, then T).  The *_drawn forms of prove and rerandomize
 * draw it on the device from a keyed ChaCha20 instead ("randomness drawn on the
 * device" below); their outputs are NOT the reference's for any rng state.
 *
 * Pointers: the *_dev entry points take DEVICE pointers (hipMalloc'ed, 16-byte
 * aligned) and enqueue on the context's stream without synchronising; the
 * un-suffixed ones take HOST pointers, stage through device memory and return
 * after the results are back.  A gs_ctx is bound to one GPU and may be used from
 * one host thread at a time.  Points must lie in the prime-order subgroups (as
 * arkworks' deserialisation guarantees).  Nothing is checked on the compute entry
 * points, and -- UNLIKE the reference, whose plain double-and-add works on any curve
 * point -- results for on-curve points OUTSIDE the subgroups are UNDEFINED here
 * (scalar multiplications use the GLV / psi-GLS endomorphisms, which act as a
 * scalar only on the r-torsion).  Three ways to be safe: decode untrusted bytes with
 * gs_wire_decode_* (validate = 1); run in-memory limbs through gs_validate_points[_dev]
 * (the same canonical / on-curve / r-torsion tests); or gs_set_option("endo", 0), which
 * runs every variable-base scalar multiplication as plain double-and-add on any curve
 * point, exactly the reference's tolerance.
 *
 * Errors: the reference panics on shape mismatch (assert_eq!, e.g.
 * src/prover/prove.rs:106-113); here every call returns a status and a shim
 * turns GS_ERR_SHAPE back into a panic.  There is NO CPU fallback: without a
 * usable GPU every compute call returns GS_ERR_DEVICE.
 */
#ifndef GS_AMD_H
#define GS_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_ctx gs_ctx;

enum { GS_CURVE_BLS12_381 = 0, GS_CURVE_BN254 = 1 };
enum { GS_PPE = 0, GS_MSMEG1 = 1, GS_MSMEG2 = 2, GS_QUAD = 3 }; /* = EquType, src/statement.rs:42-49 */
enum { GS_OK = 0, GS_ERR_SHAPE = 1, GS_ERR_DEVICE = 2, GS_ERR_ARG = 3, GS_ERR_NOCRS = 4, GS_ERR_ALLOC = 5 };

/* ---- context ---------------------------------------------------------- */
int gs_ctx_create(int curve_id, int device_ordinal, gs_ctx** out);
void gs_ctx_destroy(gs_ctx* ctx);
/* Several GPUs: one context per device ordinal, sharded by the caller, or gs_ctx_create_multi below. */
/* The context's stream (hipStream_t; NULL = the default stream), blocking or not.  ORDERING: a _dev call only enqueues.
 * Everything it enqueues -- kernels, memsets, copies, and the work it forks to the context's own non-blocking side
 * streams, which wait for the stream at the fork and are joined back into it before the call returns -- is ordered
 * after the work already on the stream and before whatever the caller enqueues there next: inputs written on the
 * stream before the call are seen, outputs may be read on the stream after it, and nothing rests on legacy
 * null-stream ordering.  A host-pointer call returns when its outputs are in the caller's memory; work the caller has
 * in flight on the stream is waited for first.  One context serves one host thread at a time; contexts of different
 * threads are independent (they share the CRS tables and the page-lock registry, both behind locks).
 * Changing the handle needs no caller-side sync: when it differs from the current one, gs_set_stream first drains the
 * context (its stream, side streams and copy queues) -- consecutive calls share named scratch buffers and are ordered
 * through the stream alone, so work in flight on the old stream must not meet the next call's on the new one.
 * Setting the same handle again costs nothing. */
int gs_set_stream(gs_ctx* ctx, void* hip_stream);
/* Planner overrides (results never change, only which kernel shapes run; tests force every shape through them):
 *   "miller_twin"  -1 planned | 0 one accumulator per Miller lane | 1 two (lines of Q shared by both G1 partners)
 *                   | 2 the same triples on a PAIR of lanes, one accumulator each, lines exchanged through LDS | 3 the
 *                   same with a DPP exchange (planned: the pair form, LDS on BLS12-381, DPP on BN254)
 *   "miller_ch"     0 planned | 1..12 pairs (triples) per Miller lane
 *   "var_tm"        0 planned | 1..8 variable-base terms per Straus lane
 *   "var_mo"        0 planned | 1, 2, 4 outputs over the same bases served by one lane's table build
 *   "var_w"         0 planned | 4, 5 window width of the Straus lanes (8 or 16 table entries per base)
 *   "var_ws_lanes"  0 = 2^19 | multiple of 64: Straus lanes per launch; bounds their table workspace (3.5 .. 28 KB
 *                   of device memory per lane), larger batches run as several launches over it
 *   "red_k"         0 planned | 1, 2, 4, 8 outputs per reduction lane (one inversion per lane)
 *   "coop_fe"       0 one lane per final exponentiation | 1 planned | 2 always the 3-lane cooperative form
 *   "line_tables"   1 CRS G2 arguments read precomputed Miller lines | 0 they are stepped like any other point
 *   "overlap"       1 independent kernels of a small batch on internal side streams | 0 one stream
 *   "var_tab"      -1 planned | 0 the verifier's Gamma^T c on Straus lanes with their own tables | 1 on window tables of
 *                   the commitment components shared by all outputs (8-bit windows; what large arities use)
 *   "var_w2"       -1 planned | 0 | 1 the G1 Straus lanes in the kernels built for TWO waves per SIMD (256 registers: the
 *                   register-only G1 point operations leave room); planned when a launch puts two waves on every SIMD
 *                   gs_mat_left_mul_com1/2 plan one term per lane ("k_var.lm") and FOLLOW the forced Straus shapes: with
 *                   "var_tm" > 1 the k terms of every output component run in balanced groups of at most var_tm terms
 *                   under "var_w", "var_mo" (all rows run over the same 2 k bases), "var_w2" and "var_ws_lanes"
 *                   ("k_var_multi<4|8>[w5][x<mo>].lm"); "var_tab" = 1 puts com1 on shared window tables of the 2 k
 *                   column components ("k_tab_build.lm", "k_var_tab8.lm"; com2 ignores it: the shared tables have no G2
 *                   caller).  That is how the tests drive those lanes with chosen bases and scalars.
 *   "endo"         1 (default) GLV / psi-GLS scalar multiplications: r-torsion points only | 0 every variable-base scalar
 *                   multiplication is a plain signed-window double-and-add lane ("k_var.plain", "k_smul_batch.plain"):
 *                   defined on ANY curve point, like the reference's Com::scalar_mul (data_structures.rs:336-342), at
 *                   ~2.5x the variable-base work.  For callers that cannot vouch for subgroup membership and do not want
 *                   to pay gs_validate_points first.  (This one changes WHICH inputs are supported, not the results on
 *                   supported ones.)  The batched verifier gs_verify_batch_rlc[_dev] and the shards of
 *                   gs_multi_verify_batch_rlc[_dev] follow it too: with 0 the rho-weighted G1 combinations of both of
 *                   its passes run as one "k_var.plain" lane per term (no "k_var_multi*" Straus groups), and the
 *                   accumulator pair and the verdict are those of endo = 1.
 *   "mixed_merge"  -1 planned (merged up to 2^14 equations per call on a 256-CU device) | 0 the parts of a mixed call run
 *                   one after the other | 1 their launches are merged
 *   "dlog_steps"    0 = 2^15 (an estimate) | giant steps one k_dlog launch walks; longer walks are several launches
 *   "dlog_fp_bits"  0 = all 35 | 1 .. 35 fingerprint bits a lookup of gs_dlog_* compares (small values force false hits,
 *                   which the confirmation rejects).  Both are test knobs without an environment twin.
 *   "locate_k"      0 planned (8, the arity of the batched verifier's own product) | 2, 4, 8 arity of the product tree of
 *                   gs_verify_batch_rlc_locate[_dev].  A test knob without an environment twin.
 *   "eq_pi"        -1 planned | 0 gs_verify_equation_rlc[_dev] pairs pi per proof (2kx pairs each, no G2 work) | 1 it folds
 *                   pi across the batch in G2 (4kx short terms and a sum per proof, 2kx pairs per call).  No environment
 *                   twin.  The accumulator pair's meaning and the verdict do not depend on it.
 * The same knobs are read ONCE at gs_ctx_create from the environment for experiments without recompiling the caller:
 * GS_MILLER_TWIN, GS_MILLER_CH, GS_VAR_TM, GS_VAR_MO, GS_VAR_W, GS_VAR_W2, GS_RED_K, GS_COOP_FE, GS_LINE_TABLES, GS_OVERLAP,
 * GS_ENDO (same values).
 * Unset = planned.  GS_COPY_THREADS (default 4): memcpy workers of the host-pointer entry points; GS_ROCTX=1: load the
 * roctx library for phase markers ("gs.prove", "gs.prove.g1", "gs.verify.miller" ...) even when no profiler mapped it.
 * Diagnostics on stderr: GS_PLAN_TRACE=1 (the verifier's Miller plan per call: mode, budget, tasks per equation, planned
 * cost of each task's lane, waves; and one line "[plan] table <name> <count> <content hash>" per task table a call uses,
 * cached or not), GS_PIPE_TRACE=1 (time line of a host-pointer call's staging, uploads and arrivals);
 * GS_PIPE_NO_DIRECT=1 stages registered arrays like pageable ones. */
int gs_set_option(gs_ctx* ctx, const char* key, int value);
/* hipStreamSynchronize on the context's stream, then on its side streams.  Every call joins what it forked to the
 * side streams back into the context's stream before it returns, so the first wait already covers them; the second
 * makes that hold after a call that failed half way.  After gs_sync the outputs of every _dev call made so far may be
 * read from any stream or copied with a blocking hipMemcpy. */
int gs_sync(gs_ctx* ctx);
/* Page-locked caller memory.  The host-pointer entry points below (gs_prove_batch, gs_verify_batch, the mixed and the
 * Statement calls, gs_multi_*) stage pageable arrays through a pinned buffer of their own (one memcpy per array and
 * direction on worker threads).  An array that lies inside a range registered HERE is moved by DMA straight from / to
 * the caller's memory: no staging copy, uploads start at once (profiles/r3/host_path_rate.txt).  A Rust caller
 * registers the Vecs it reuses across calls once (registration costs about as much as copying the buffer a few times).
 * [prove.rs:29-52 / verifier.rs:18-21 take slices; this is the cheap way to hand them over]
 * Only ranges registered through this call count: memory page-locked by other means (hipHostMalloc, another library's
 * hipHostRegister) is staged like pageable memory -- the runtime cannot tell such memory from ranges it has pinned
 * itself for an earlier pageable copy, and those may be mapped read-only or belong to a buffer freed since.
 * Registrations are per process, not per context: they outlive gs_ctx_destroy and end with gs_host_unregister (any live
 * context may be passed).  gs_host_unregister first drains EVERY live context of the process (compute stream, side
 * streams and the copy queues -- the shards of a gs_multi context included): no DMA touches the range afterwards.  GS_ERR_ARG: null / empty / already registered (here or
 * elsewhere) / unknown. */
int gs_host_register(gs_ctx* ctx, void* ptr, size_t bytes);
int gs_host_unregister(gs_ctx* ctx, void* ptr);
/* The easy way to the same: gs_host_alloc returns `bytes` of host memory on a mapping of its own (page-aligned, never
 * part of the allocator's heap), every page already touched (no first-touch faults inside a call: result arrays made
 * per call cost 27-35 ms of them at 2^16), page-locked and registered -- a shim that keeps its Vec-like buffers in such
 * memory gets DMA-direct transfers with one call per buffer.  gs_host_free drains every context, unregisters and unmaps.
 * (What a Rust shim would wrap in a Drop type: INTEGRATION.md.) */
int gs_host_alloc(gs_ctx* ctx, size_t bytes, void** out);
int gs_host_free(gs_ctx* ctx, void* ptr);
const char* gs_last_error(gs_ctx* ctx);
const char* gs_version(void);
/* sizes in bytes of the boundary PODs for a curve: out[0..5] = Fq, Fr, G1, G2, GT, CRS */
int gs_sizes(int curve_id, size_t out[6]);

/* CRS (host pointer): uploads, derives W1 = u[1]+(O,g1), W2 = v[1]+(O,g2) and
 * builds the fixed-base window tables (16-bit windows: 1.8 GB of device memory) and the Miller
 * line tables of its G2 elements on the device.  The tables are immutable and SHARED: every context of the process
 * that installs the same CRS bytes on the same device uses one copy (reference-counted; freed with the last context),
 * so a pool of worker contexts costs 1.8 GB per device, not per worker.
 * What IS per context (grow-only, sized by the largest batch the context has seen; freed by gs_ctx_destroy):
 *   - engine scratch: scalar pool, Jacobian partial slots, Miller partials: ~1 GB at 2^16 PPEs of 4 + 4 variables;
 *   - the Straus lanes' workspaces (affine tables + the Jacobian staging of their build): 9 .. 70 KB per lane, at most
 *     2 x (SIMDs of the device) x 64 lanes per side ("var_ws_lanes" lowers that): <= 9.2 GB for the largest lane
 *     shape (G2, 8 terms, 5-bit windows), ~6 GB in total for the 2^16 PPE shapes;
 *   - host-pointer entry points only: a pinned host buffer and device staging of the call's input + output bytes each
 *     (a 2^16 PPE 4x4: 0.45 GB for prove, 0.37 GB for verify; grow-only, so a context that does both holds 0.45 GB);
 *   - large arities only: the shared per-base window tables, N x 2 m bases x 128 entries (affine + Jacobian staging:
 *     36 KB per base in G1; planned only while that stays below 8 GB);
 *   - mixed calls: the above once per PART (the parts' scratch is live at the same time).
 * A pool of W worker contexts on one GPU therefore costs 1.8 GB + W x (the above for the workers' batch size).
 * ON A LIVE CONTEXT the call may be repeated with another CRS.  ORDERING: it first drains the context (stream, side
 * streams, copy queues), so calls in flight finish under the CRS they were made with before this context's reference
 * on the old tables goes (the tables are freed when no other context holds them); it returns when the new tables are
 * built, and synchronises the context's stream on the way.  The extraction key is forgotten and its digit streams
 * zeroed (a key belongs to the CRS it was checked against: gs_extract_* give GS_ERR_ARG until gs_set_extraction_key is
 * called again, also when the same CRS comes back).  The tables of gs_dlog_prepare are not tied to the CRS and stay.
 * Other contexts that hold the old CRS are not touched. */
int gs_set_crs(gs_ctx* ctx, const void* crs_host);

/* CRS of the reference's shape (src/generator.rs:81-118, binding key :48-60) from caller-drawn values:
 * generators p1 (G1), p2 (G2) and scalars[4] = a1, a2, t1, t2 (Fr):
 *   u = [(p1, a1 p1), (t1 p1, t1 a1 p1)],  v = [(p2, a2 p2), (t2 p2, t2 a2 p2)],  g1 = p1, g2 = p2, gt = e(p1, p2).
 * Host pointers; the result is written to crs_out (CRS layout) and NOT installed (call gs_set_crs). */
int gs_crs_generate(gs_ctx* ctx, const void* p1_g1, const void* p2_g2, const void* scalars_fr4, void* crs_out);
/* The simulation ("hiding") key of src/generator.rs:65-77 (dead code there): as above with
 *   u[1] = (t1 p1, t1 a1 p1 - p1),  v[1] = (t2 p2, t2 a2 p2 - p2). */
int gs_crs_generate_hiding(gs_ctx* ctx, const void* p1_g1, const void* p2_g2, const void* scalars_fr4, void* crs_out);

/* ---- commit (src/prover/commit.rs) -------------------------------------- */
/* c_i = iota1(X_i) + r_i0 u0 + r_i1 u1   (commit.rs:78-100; N=1 is commit_G1 :59-75) */
int gs_commit_g1_dev(gs_ctx*, size_t count, const void* x_g1, const void* rand_fr2, void* out_com1);
int gs_commit_g2_dev(gs_ctx*, size_t count, const void* y_g2, const void* rand_fr2, void* out_com2);
/* c_i = x_i W1 + r_i u0                  (commit.rs:125-156, 225-256) */
int gs_commit_fr_b1_dev(gs_ctx*, size_t count, const void* x_fr, const void* rand_fr, void* out_com1);
int gs_commit_fr_b2_dev(gs_ctx*, size_t count, const void* y_fr, const void* rand_fr, void* out_com2);
int gs_commit_g1(gs_ctx*, size_t count, const void* x_g1, const void* rand_fr2, void* out_com1);
int gs_commit_g2(gs_ctx*, size_t count, const void* y_g2, const void* rand_fr2, void* out_com2);
int gs_commit_fr_b1(gs_ctx*, size_t count, const void* x_fr, const void* rand_fr, void* out_com1);
int gs_commit_fr_b2(gs_ctx*, size_t count, const void* y_fr, const void* rand_fr, void* out_com2);

/* ---- prove (src/prover/prove.rs) ---------------------------------------- */
/* Batch of N independent equations of one type and shape over the shared CRS.
 * xcoms/ycoms may be NULL (prove only) or receive the commitments
 * (commit_and_prove).  pi: N*kx Com2, theta: N*ky Com1.
 * Host-pointer forms (no _dev suffix; what a Rust caller of prove.rs:29-52 / verifier.rs:18-21 holds): the arrays are
 * staged through a grow-only PINNED buffer by a few memcpy workers, uploaded on a copy stream array by array, and the
 * kernels wait only for the arrays they read (scalars before the preparation kernel, G1 arguments before the G1 side,
 * G2 arguments before the G2 side / the Miller loop), so most of the transfer runs under kernels; outputs come back
 * the same way.  Per context: pinned staging = the largest call's input + output bytes (2^16 PPE 4x4:
 * 0.45 GB for prove, 0.37 GB for verify; 0.83 GB is what ONE prove + verify step moves across PCIe, not what is held),
 * device staging the same, plus the engine's scratch (section "memory" of DESIGN.md). */
int gs_prove_batch_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                       const void* B, const void* Gamma, const void* R, const void* S, const void* T, void* xcoms,
                       void* ycoms, void* pi, void* theta);
int gs_prove_batch(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                   const void* B, const void* Gamma, const void* R, const void* S, const void* T, void* xcoms,
                   void* ycoms, void* pi, void* theta);

/* A Statement (src/statement.rs:24-28,109: "a list of equations ... defined with respect to the list of variables that
 * span across ALL equations"): E equations of ONE type over the SAME m + n variables.  The variables are committed ONCE
 * (X[m], Y[n] with randomness R[m][kx], S[n][ky]: exactly gs_commit_*), every equation e gets its own proof from its
 * A[e], B[e], Gamma[e] and T[e][ky][kx] -- what calling Provable::prove E times with the same commitments does
 * (prove.rs:92-171 ...).  xcoms[m] / ycoms[n] may be NULL (already committed).  pi: E*kx Com2, theta: E*ky Com1. */
int gs_prove_statement_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                           const void* B, const void* Gamma, const void* R, const void* S, const void* T, void* xcoms,
                           void* ycoms, void* pi, void* theta);
int gs_prove_statement(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                       const void* B, const void* Gamma, const void* R, const void* S, const void* T, void* xcoms,
                       void* ycoms, void* pi, void* theta);

/* ---- rerandomize (no witness) --------------------------------------------- */
/* From commitments xcoms[N][m] (Com1), ycoms[N][n] (Com2) and proofs pi[N][kx], theta[N][ky] of N equations, and fresh
 * randomness R'[N][m][kx], S'[N][n][ky], T'[N][ky][kx] (the layouts of gs_prove_batch), new commitments and proofs
 * that verify against the same equations, WITHOUT the witness X, Y:
 *   c'_i   = c_i + sum_a R'_ia U_x,a                 d'_j = d_j + sum_b S'_jb V_y,b
 *   pi'    = pi + R'^T iota2(B) + (R'^T Gamma) d + (R'^T Gamma S' - T'^T) V_y        (d = the OLD commitments)
 *   theta' = theta + S'^T iota1(A) + (S'^T Gamma^T) c + T' U_x                        (c = the OLD commitments)
 * U_x = (u0, u1) for G1 variables, (u0) for scalar ones; V_y likewise with v; iota1/iota2 are the maps the prover
 * applies to A and B.  Starting from gs_prove_batch(X, Y, R, S, T), the output is BYTE-IDENTICAL to
 * gs_prove_batch(X, Y, R + R', S + S', T + T' + S'^T Gamma^T R) (commitments included), and the verifier's verdict is
 * unchanged: valid proofs stay valid, invalid ones stay invalid (nothing is verified here).
 * RANDOMNESS: R', S', T' must be uniform, fresh and secret.  Reused or predictable values make the output linkable to
 * its input.
 * INPUTS: rerandomized proofs usually arrive from another party.  Points outside the prime-order subgroups give
 * UNDEFINED results, exactly as on the other compute entry points (see the top of this file): decode them with
 * gs_wire_decode_* (validate = 1), run them through gs_validate_points[_dev], or set gs_set_option("endo", 0).
 * Outputs must not overlap any input or each other: the host form returns GS_ERR_ARG if they do; for the _dev form it
 * is the caller's contract (results are undefined otherwise).  Shapes and errors as gs_prove_batch; N = 0 is a no-op. */
int gs_rerandomize_batch_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                             const void* Gamma, const void* xcoms, const void* ycoms, const void* pi,
                             const void* theta, const void* R, const void* S, const void* T, void* xcoms_out,
                             void* ycoms_out, void* pi_out, void* theta_out);
int gs_rerandomize_batch(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                         const void* Gamma, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                         const void* R, const void* S, const void* T, void* xcoms_out, void* ycoms_out, void* pi_out,
                         void* theta_out);
/* A Statement (gs_prove_statement's shape): xcoms[m], ycoms[n], R'[m][kx], S'[n][ky] (and xcoms_out / ycoms_out) are
 * ONE shared copy, updated once; A, B, Gamma, pi, theta and T'[E][ky][kx] are per equation.  The output equals
 * gs_prove_statement(X, Y, R + R', S + S', T_e + T'_e + S'^T Gamma_e^T R) for every equation e. */
int gs_rerandomize_statement_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B,
                                 const void* Gamma, const void* xcoms, const void* ycoms, const void* pi,
                                 const void* theta, const void* R, const void* S, const void* T, void* xcoms_out,
                                 void* ycoms_out, void* pi_out, void* theta_out);
int gs_rerandomize_statement(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B,
                             const void* Gamma, const void* xcoms, const void* ycoms, const void* pi,
                             const void* theta, const void* R, const void* S, const void* T, void* xcoms_out,
                             void* ycoms_out, void* pi_out, void* theta_out);

/* ---- extract (the binding key opens commitments) ---------------------------- */
/* The CRS of gs_crs_generate is u0 = (p1, a1 p1), u1 = t1 u0 (and v with a2, t2, p2).  Whoever drew a1, a2 can open
 * ANY commitment to the witness it binds:
 *   G1 variable  c = (O, X) + r0 u0 + r1 u1  ->  c.1 - a1 c.0 = X
 *   Fr variable  c = x W1 + r u0             ->  c.1 - a1 c.0 = x p1   (the witness's IMAGE: recovering x from it is a
 *                                                 discrete logarithm: gs_extract_scalar_* below, for short x)
 * and likewise in G2 with a2.  On the hiding key (gs_crs_generate_hiding) u1.1 = t1 a1 p1 - p1 and nothing can be
 * extracted; that key is refused.
 *
 * gs_set_extraction_key: a1a2_fr2 is a HOST pointer to a1, a2 (two Fr, Montgomery limbs); NULL forgets the key.  Needs
 * an installed CRS (GS_ERR_NOCRS) and checks u[0].1 == a1 u[0].0, u[1].1 == a1 u[1].0, v[0].1 == a2 v[0].0 and
 * v[1].1 == a2 v[1].0 on the device: a wrong key or a hiding CRS returns GS_ERR_ARG, gs_last_error names the check that
 * failed, and no key is installed (an earlier one is gone too).  The call synchronises the stream.  gs_set_crs forgets
 * the key.  The key is a SECRET: the context keeps it only as digit streams in device memory, which are zeroed (as is
 * the staged copy of the key itself) when the key is cleared or replaced, on gs_set_crs and on gs_ctx_destroy.  The
 * caller's own buffer is the caller's to wipe.
 *
 * gs_extract_g1 / gs_extract_g2: out[i] = coms[i].1 - a coms[i].0 for count Com1 (a = a1, out in G1) or Com2 (a = a2,
 * out in G2) elements, normalised affine, the identity all-zero bytes.  It is a map on ALL of Com, not only on honest
 * commitments.  count = 0 is a no-op; GS_ERR_ARG while no key is installed; out must not overlap coms (GS_ERR_ARG on
 * the _dev form; the host form stages).  The _dev forms enqueue on the context's stream without synchronising.
 * INPUTS: opened commitments usually come from ANOTHER PARTY.  As on the other compute entry points (top of this
 * file) nothing is checked, and with "endo" = 1 (the default) components outside the prime-order subgroups give
 * UNDEFINED results: decode them with gs_wire_decode_* (validate = 1), run them through gs_validate_points[_dev], or
 * set gs_set_option("endo", 0), under which the result is c.1 - a c.0 for ANY pair of curve points. */
int gs_set_extraction_key(gs_ctx*, const void* a1a2_fr2);
int gs_extract_g1_dev(gs_ctx*, size_t count, const void* coms_com1, void* out_g1);
int gs_extract_g2_dev(gs_ctx*, size_t count, const void* coms_com2, void* out_g2);
int gs_extract_g1(gs_ctx*, size_t count, const void* coms_com1, void* out_g1);
int gs_extract_g2(gs_ctx*, size_t count, const void* coms_com2, void* out_g2);

/* ---- simulate (the hiding key's trapdoor answers equations without a witness) ---------------------------------------
 * The CRS of gs_crs_generate_hiding is u0 = (p1, a1 p1), u1 = t1 u0 - (O, p1) (and v with a2, t2, p2), so that
 *   W1 = u1 + (O, g1) = t1 u0        W2 = v1 + (O, g2) = t2 v0.
 * Whoever drew t1, t2 can produce commitments and proofs for an equation WITHOUT ANY WITNESS -- also for an equation no
 * witness satisfies -- and they are distributed exactly like honest ones (perfect zero-knowledge).  That is the simulator
 * of the security experiments of credentials, ballots and shuffles, and a way to load a verifier pipeline without real
 * witnesses.  On the binding key (gs_crs_generate) W1 != t1 u0 and nothing can be simulated; that key is refused.
 *
 * gs_set_simulation_key: t1t2_fr2 is a HOST pointer to t1, t2 (two Fr, Montgomery limbs); NULL forgets the key.  Needs an
 * installed CRS (GS_ERR_NOCRS) and checks u[1] + (O, g1) == t1 u[0] and v[1] + (O, g2) == t2 v[0], component by component,
 * on the device with plain double-and-add (the verdict is defined whatever the CRS holds): a binding CRS or a wrong key
 * returns GS_ERR_ARG, gs_last_error names the check that failed, and no key is installed (an earlier one is gone too).
 * The call synchronises the stream.  gs_set_crs forgets the key (also when the same CRS comes back).  The key is a
 * SECRET, handled as gs_set_extraction_key handles its own: the context's copy and the staged copy are zeroed on the
 * stream when the key is cleared, replaced or refused, on gs_set_crs and on gs_ctx_destroy; the simulator's scalar pool
 * (it holds -t2, t2 b_i + ... and the like) is zeroed on the stream after the last kernel of every call that reads it.
 * The caller's own buffer is the caller's to wipe.
 *
 * gs_simulate_batch: N equations of one type and shape, A, B, Gamma, target as gs_verify_batch takes them, and
 *   Rc[N][m][kx]   the coordinates of the x-commitments in the basis u     (layout of gs_prove_batch's R)
 *   Sc[N][n][ky]   the same for y in the basis v                           (layout of S)
 *   Tf[N][ky][kx]  the free proof scalars                                  (layout of T)
 * all UNIFORM, FRESH and SECRET: randomness is an input here as everywhere.  Outputs (xcoms / ycoms may be NULL):
 *   c_i = sum_a Rc_ia u_a          d_j = sum_b Sc_jb v_b      byte for byte what gs_prove_batch writes for the all-identity
 *                                                             (all-zero) witness with R = Rc, S = Sc
 *   GS_QUAD    theta = Tf[0][0] u0,  pi = pi' v0 with
 *              pi' = t2 sum_i Rc_i b_i + t1 sum_j a_j Sc_j + sum_ij Rc_i Gamma_ij Sc_j - t t1 t2 - Tf[0][0]
 *   GS_MSMEG1  pi_k = Tf[0][k] v0,  theta = (O, V) + (sum_i e_i Rc_i0 - Tf[0][0]) u0 + (sum_i e_i Rc_i1 - Tf[0][1]) u1
 *              with e_i = t2 b_i + sum_j Gamma_ij Sc_j and V = sum_j Sc_j A_j - t2 T
 *   GS_MSMEG2  theta_l = Tf[l][0] u0,  pi = (O, V) + (sum_j f_j Sc_j0 - Tf[0][0]) v0 + (sum_j f_j Sc_j1 - Tf[1][0]) v1
 *              with f_j = t1 a_j + sum_i Rc_i Gamma_ij and V = sum_i Rc_i B_i - t1 T
 *   GS_PPE     REFUSED (GS_ERR_ARG): iota_T(t) of a general target t in GT has no preimage the simulator could pair its
 *              way to, and a PPE with target one is already simulated by gs_prove_batch at the identity witness.
 * gs_verify_batch accepts the output under the hiding CRS for ANY A, B, Gamma, target.  For a satisfied equation the
 * honest proof under the hiding CRS equals the simulated one at the corresponding coordinates -- a G1 variable
 * X_i = xi_i g1 committed with R_i sits at Rc_i = (R_i0 + xi_i t1, R_i1 - xi_i), a scalar x_i at Rc_i = R_i + x_i t1
 * (likewise Sc with t2), Tf = the v0- (u0-) coordinates of the honest pi_k (theta_l) -- BYTE FOR BYTE.
 * gs_simulate_statement: E equations over ONE set of commitments: Rc[m][kx], Sc[n][ky], xcoms[m], ycoms[n] are one copy,
 * written once; A, B, Gamma, target, Tf[E][ky][kx], pi and theta are per equation; gs_verify_statement accepts.
 * Errors: GS_ERR_ARG while no key is installed, for GS_PPE, and inside a mixed call; the host forms return GS_ERR_ARG when
 * an output overlaps an input or another output (for the _dev forms that is the caller's contract); shapes and the
 * remaining errors are those of gs_prove_batch; N == 0 is a no-op.  The _dev forms only enqueue on the context's stream.
 * The multi-GPU handles (gs_multi_*) have NO counterpart: use a shard's context (gs_multi_ctx).  A and B come from the
 * equation; as on the other compute entry points nothing is checked and points outside the prime-order subgroups give
 * undefined results unless "endo" = 0, under which the variable-base lanes run plain ("k_var.plain").  "var_tm",
 * "var_w", "var_w2", "var_ws_lanes" and "red_k" act as they do elsewhere.
 * How it is computed: one lane of Fr arithmetic per equation ("k_prep_sim"; the trapdoor is read through
 * scalar loads), every output component one fixed-base lane on the CRS tables ("k_fix.sm1|.sm2"), V as n + 1 (m + 1)
 * Straus terms ("k_var*.sm1|.sm2"), then the usual reductions ("k_red.sm1|.sm2"; a Statement's commitments: ".sc1|.sc2").
 * WHEN TO CALL IT: the simulator does no more group work than gs_prove_batch with commitments on the same shape (the same
 * commitment lanes with fewer terms, n + 1 or m + 1 Straus terms against m + n), so wherever a test bench or a trapdoor
 * setup would otherwise invent witnesses and prove, it may simulate instead.  Measured (tools/sim_rate.py,
 * profiles/simulate/rate.json, DESIGN.md 6.9: BLS12-381, 4 x 4, one MI355X, device-resident, median of 7, the two entries
 * alternating), ms per call, this entry against gs_prove_batch_dev on the same shape -- MSMEG1: 2.90 against 3.53 at
 * N = 2^12 (ratio 0.82), 14.96 against 23.15 at 2^16 (0.65); QuadEqu: 0.94 against 1.54 (0.61) and 7.05 against 13.08
 * (0.54); MSMEG2 at 2^16: 25.16 against 35.39 (0.71). */
int gs_set_simulation_key(gs_ctx*, const void* t1t2_fr2);
int gs_simulate_batch_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B, const void* Gamma,
                          const void* target, const void* Rc, const void* Sc, const void* Tf, void* xcoms, void* ycoms,
                          void* pi, void* theta);
int gs_simulate_batch(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B, const void* Gamma,
                      const void* target, const void* Rc, const void* Sc, const void* Tf, void* xcoms, void* ycoms,
                      void* pi, void* theta);
int gs_simulate_statement_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B,
                              const void* Gamma, const void* target, const void* Rc, const void* Sc, const void* Tf,
                              void* xcoms, void* ycoms, void* pi, void* theta);
int gs_simulate_statement(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B, const void* Gamma,
                          const void* target, const void* Rc, const void* Sc, const void* Tf, void* xcoms, void* ycoms,
                          void* pi, void* theta);

/* ---- randomness drawn on the device (a keyed, counter-addressed ChaCha20) --------------------------------------------
 * The entry points above take their secret scalars R, S, T (and the verifiers their rho) as arrays the caller has drawn.
 * These draw them in device memory instead: nothing is drawn on a host thread and nothing is staged across PCIe.
 *
 * The generator is the ChaCha20 block function of RFC 8439 section 2.3 (20 rounds, 32-bit block counter in state word
 * 12, 96-bit nonce in words 13..15) under a 32-byte key (state words 4..11, little-endian) and the nonce
 * LE32(domain) || LE64(stream).  The block counter is the element's block index and there is no running state: element
 * i of a draw is a pure function of (key, domain, stream, i), whatever the launch shape, so a shard draws its slice of a
 * global array by passing `first`.
 *   Fr   one block per scalar, element i = block first + i.  The 64 output bytes are a 512-bit little-endian integer v;
 *        the scalar is v mod r (bias below 2^-256 on both curves), written as every entry point takes an Fr (4 u64 limbs
 *        of x 2^256 mod r).
 *   rho  eight little-endian u64 per block under the domain GS_RAND_RHO: element j = word (first + j) mod 8 of block
 *        (first + j) div 8.  A zero word is replaced by 1 (bias 2^-64): the rho contract of the *_rlc verifiers demands
 *        non-zero exponents and their _dev forms cannot look.
 * Domains: the library's own are the enum below; a caller's own draws use domains >= GS_RAND_USER.  gs_rand_fr[_dev]
 * accepts ANY domain, the library's included -- that is what defines the drawn entries and makes them testable.
 *
 * gs_rand_set_key: key32 is a HOST pointer to 32 bytes; NULL forgets the key.  The key is a SECRET, handled as
 * gs_set_simulation_key handles its own: it goes from the caller's buffer straight into the context's device copy (the
 * library keeps no staged copy that could outlive the call), and that copy is zeroed on gs_rand_set_key(NULL), on
 * replacement, when the upload fails and on gs_ctx_destroy.  It is not tied to the CRS (no CRS is needed, and
 * gs_set_crs leaves it alone).  The call synchronises the stream.  The caller's own buffer is the caller's to wipe.
 *
 * THE CONTRACT.  The key comes from a CSPRNG.  A (key, stream) pair is used for ONE call of ONE operation: a reused
 * pair repeats the randomness, which links the proofs and breaks witness-indistinguishability (two proofs under the same
 * R, S, T reveal differences of witnesses).  A rho stream is drawn AFTER the batch to be verified is fixed, and the key
 * stays secret until the verdict is out: whoever knows rho before choosing the proofs can cancel a forgery.
 *
 * gs_rand_fr / gs_rand_rho write `count` elements to out (host pointer; _dev: device pointer, only enqueued).
 * Errors: GS_ERR_ARG while no key is installed, for a null out, and inside a mixed call.  GS_ERR_SHAPE when the draw
 * would need a block counter >= 2^32 -- first + count > 2^32 for Fr, (first + count + 7) div 8 > 2^32 for rho; the
 * counter never wraps and nothing is written.  count == 0 is a no-op.
 *
 * The DRAWN forms of prove and rerandomize take a stream number where their siblings take R, S, T:
 *   gs_prove_batch_drawn_dev(..., stream, R_out, S_out, T_out, ...) writes, byte for byte, what gs_prove_batch_dev writes for
 *     R = gs_rand_fr(GS_RAND_PROVE_R, stream, 0, N m kx)   S = gs_rand_fr(GS_RAND_PROVE_S, stream, 0, N n ky)
 *     T = gs_rand_fr(GS_RAND_PROVE_T, stream, 0, N ky kx)
 *   in the layouts of gs_prove_batch (element index = flat array index).  The statement forms draw R[m][kx], S[n][ky]
 *   once and T[E][ky][kx]; the rerandomize forms are the same over GS_RAND_RERAND_R/S/T.  The host forms compute what
 *   the _dev forms compute.
 * R_out, S_out, T_out may each be NULL: a prover that later opens or rerandomizes needs them, a mix server does not.
 * Arrays not asked for live in the context's scratch and are zeroed on the stream behind the last kernel that reads
 * them.  In the host forms R, S, T are never staged in: they come back with the other outputs when asked for.
 * Errors: GS_ERR_ARG while no key is installed, inside a mixed call, and (host forms) when an output overlaps an input or
 * another output; GS_ERR_SHAPE when one of the three arrays has more than 2^32 scalars; N == 0 is a no-op; shapes and
 * the remaining errors are those of gs_prove_batch / gs_rerandomize_batch.
 * OUT OF SCOPE: there are no drawn forms of gs_simulate_*, of the mixed calls or of the gs_multi_* handles.  Those
 * callers compose gs_rand_fr_dev (first = their global offset, on a shard's context) with the existing _dev entries.
 * How it is computed: "k_rand_fr" (one lane per scalar: the block, then two 8-limb Montgomery products
 * by R^2 and R^3 mod r and one modular addition) and "k_rand_rho" (one lane per block), 256-thread blocks, the key read
 * through scalar loads; then the kernels of gs_prove_batch_dev / gs_rerandomize_batch_dev, unchanged.
 * WHEN TO CALL IT: whenever the caller does not need the reference's outputs for a given rng state (parity: the entries
 * that take R, S, T).  Measured (tools/rand_rate.py, profiles/rand/rate.json, DESIGN.md 6.10: one MI355X, BLS12-381,
 * PPE 4 x 4, median of 7 after a warm-up, the entries alternating, every entry writing into the same preallocated
 * arrays), ms per call.  The generator alone, one call with launch and sync: the 20 N scalars of a prove 0.031 at
 * N = 2^12 and 0.081 at 2^16 (1.31 M scalars), the 4 N exponents of a batched check 0.026 and 0.019.  Host pointers,
 * gs_prove_batch_drawn with R_out = S_out = T_out = NULL against gs_prove_batch given ready-made arrays: 9.41 against
 * 9.53 at 2^12 (ratio 0.987, the yardstick's own spread 0.063), 71.69 against 73.01 at 2^16 (0.982, spread 0.025; 41.9 MB
 * of scalars not staged); with all three returned 9.48 (0.995) and 72.30 (0.990).  Device pointers, against
 * gs_prove_batch_dev: 8.01 against 7.90 at 2^12 (1.014, spread 0.051) and 65.06 against 64.75 at 2^16 (1.005, spread
 * 0.009); returned 8.02 (1.016) and 64.93 (1.003): three more launches and the zeroing, inside the yardstick's spread
 * in every row.  The drawn entry is not slower than its sibling anywhere it was measured; what it saves the CALLER --
 * drawing 20 N scalars on a host thread before the call -- is not in these numbers and was not measured. */
enum {
  GS_RAND_PROVE_R = 0x0101, GS_RAND_PROVE_S = 0x0102, GS_RAND_PROVE_T = 0x0103,
  GS_RAND_RERAND_R = 0x0201, GS_RAND_RERAND_S = 0x0202, GS_RAND_RERAND_T = 0x0203,
  GS_RAND_RHO = 0x0301,
  GS_RAND_USER = 0x10000 /* callers' own domains start here */
};
int gs_rand_set_key(gs_ctx*, const void* key32);
int gs_rand_fr_dev(gs_ctx*, uint32_t domain, uint64_t stream, uint64_t first, size_t count, void* out_fr);
int gs_rand_fr(gs_ctx*, uint32_t domain, uint64_t stream, uint64_t first, size_t count, void* out_fr);
int gs_rand_rho_dev(gs_ctx*, uint64_t stream, uint64_t first, size_t count, uint64_t* out);
int gs_rand_rho(gs_ctx*, uint64_t stream, uint64_t first, size_t count, uint64_t* out);
int gs_prove_batch_drawn_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                             const void* B, const void* Gamma, uint64_t stream, void* R_out, void* S_out, void* T_out,
                             void* xcoms, void* ycoms, void* pi, void* theta);
int gs_prove_batch_drawn(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                         const void* B, const void* Gamma, uint64_t stream, void* R_out, void* S_out, void* T_out,
                         void* xcoms, void* ycoms, void* pi, void* theta);
int gs_prove_statement_drawn_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y,
                                 const void* A, const void* B, const void* Gamma, uint64_t stream, void* R_out,
                                 void* S_out, void* T_out, void* xcoms, void* ycoms, void* pi, void* theta);
int gs_prove_statement_drawn(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                             const void* B, const void* Gamma, uint64_t stream, void* R_out, void* S_out, void* T_out,
                             void* xcoms, void* ycoms, void* pi, void* theta);
int gs_rerandomize_batch_drawn_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                                   const void* Gamma, const void* xcoms, const void* ycoms, const void* pi,
                                   const void* theta, uint64_t stream, void* R_out, void* S_out, void* T_out,
                                   void* xcoms_out, void* ycoms_out, void* pi_out, void* theta_out);
int gs_rerandomize_batch_drawn(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                               const void* Gamma, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                               uint64_t stream, void* R_out, void* S_out, void* T_out, void* xcoms_out, void* ycoms_out,
                               void* pi_out, void* theta_out);
int gs_rerandomize_statement_drawn_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B,
                                       const void* Gamma, const void* xcoms, const void* ycoms, const void* pi,
                                       const void* theta, uint64_t stream, void* R_out, void* S_out, void* T_out,
                                       void* xcoms_out, void* ycoms_out, void* pi_out, void* theta_out);
int gs_rerandomize_statement_drawn(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B,
                                   const void* Gamma, const void* xcoms, const void* ycoms, const void* pi,
                                   const void* theta, uint64_t stream, void* R_out, void* S_out, void* T_out,
                                   void* xcoms_out, void* ycoms_out, void* pi_out, void* theta_out);

/* ---- dlog (bounded scalar witnesses back from their images) --------------- */
/* gs_extract_* opens a committed SCALAR to its image x * generator.  The scalars committed under Groth-Sahai (amounts,
 * votes, attribute values, indices) are short; these calls recover x in [0, 2^bits) by baby-step giant-step:
 *   found[i] = 1, out[i] = x_i   when 0 <= x_i < 2^bits with x_i * base == pts[i] exists; out is an Fr in the form
 *                                gs_commit_fr_b1 takes, so an opened commitment returns the bytes that were committed
 *   found[i] = 0, out[i] = 0     otherwise
 * The answer is exact: a reported x has been confirmed by x * base == pts[i] on full coordinates.  pts may be ANY curve
 * points: one outside <base> (a cofactor component, say) gives found = 0.  An input off the curve has an undefined
 * verdict, but every loop is bounded and the call returns.
 *
 * gs_dlog_prepare builds the baby-step table j * base, j = 1 .. 2^log2_table, for group 1 (G1) or 2 (G2) on the device:
 * base_host is a HOST pointer to one affine point.  One table per group per context; a second call for the group
 * replaces the table (the old one is freed first), gs_ctx_destroy frees them.  The table is PUBLIC data: it is not
 * tied to the CRS and gs_set_crs leaves it alone.  MEMORY: 2^(log2_table + 1) slots of 8 bytes (load factor <= 1/2),
 * i.e. 256 MB at log2_table = 24.  GS_ERR_ARG for the identity as base, a group other than 1 | 2 or log2_table outside
 * [2, 28]; GS_ERR_ALLOC when the table does not fit.  The call synchronises the stream.  The base is meant to generate
 * the group the points live in (the CRS generator: prime order r).  A base of SMALL order is accepted, but multiples
 * i * 2^(log2_table+1) * base of the walk that fall on the identity are not treated specially, so found may be 0 for an
 * x that exists; a reported x is still always a confirmed one.
 * Kernel profile names (gs_prof_get): "k_dlog_table.g1|g2" and "k_dlog_steps.g1|g2" once per gs_dlog_prepare (the
 * baby-step table and the few launch-uniform giant steps), "k_dlog.g1|g2" once per launch of the walk.
 *
 * gs_dlog_g1 / gs_dlog_g2 (host pointers) and their _dev forms (device pointers, enqueued on the context's stream
 * without synchronising): a lane walks 2^(bits - log2_table - 1) giant steps at worst, about 6 Fq multiplications each
 * in G1.  GS_ERR_ARG when no table is prepared for the group, when bits is outside [1, 48], when
 * bits > log2_table + 25 (more than 2^24 giant steps per lane: gs_last_error names the table size that is needed),
 * when out_fr, found_u8 and the input overlap, and inside a mixed call.  count = 0 is a no-op.
 *
 * gs_extract_scalar_b1 / _b2: gs_extract_g1 / _g2 into context scratch, then the walk over the images.  Needs the
 * extraction key (refusals as gs_extract_*) and a table prepared for the group with the CRS generator (g1_gen /
 * g2_gen) as base; with any other base the confirmation gives found = 0, never a wrong x.
 * The multi-GPU handles (gs_multi_*) have no counterpart of these calls: use a shard's context (gs_multi_ctx). */
int gs_dlog_prepare(gs_ctx*, int group /* 1 | 2 */, const void* base_host, unsigned log2_table);
int gs_dlog_g1_dev(gs_ctx*, size_t count, const void* pts_g1, unsigned bits, void* out_fr, void* found_u8);
int gs_dlog_g2_dev(gs_ctx*, size_t count, const void* pts_g2, unsigned bits, void* out_fr, void* found_u8);
int gs_dlog_g1(gs_ctx*, size_t count, const void* pts_g1, unsigned bits, void* out_fr, void* found_u8);
int gs_dlog_g2(gs_ctx*, size_t count, const void* pts_g2, unsigned bits, void* out_fr, void* found_u8);
int gs_extract_scalar_b1_dev(gs_ctx*, size_t count, const void* coms_com1, unsigned bits, void* out_fr, void* found_u8);
int gs_extract_scalar_b2_dev(gs_ctx*, size_t count, const void* coms_com2, unsigned bits, void* out_fr, void* found_u8);
int gs_extract_scalar_b1(gs_ctx*, size_t count, const void* coms_com1, unsigned bits, void* out_fr, void* found_u8);
int gs_extract_scalar_b2(gs_ctx*, size_t count, const void* coms_com2, unsigned bits, void* out_fr, void* found_u8);

/* ---- verify (src/verifier.rs) ------------------------------------------- */
/* ok[i] = 1 iff equation i verifies; exact reference semantics (four GT cell
 * equalities per equation). */
int gs_verify_batch_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                        const void* Gamma, const void* target, const void* xcoms, const void* ycoms, const void* pi,
                        const void* theta, uint8_t* ok);
int gs_verify_batch(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B, const void* Gamma,
                    const void* target, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                    uint8_t* ok);
/* ok[e] = 1 iff equation e of a Statement verifies against the SHARED commitments xcoms[m], ycoms[n]. */
int gs_verify_statement_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B,
                            const void* Gamma, const void* target, const void* xcoms, const void* ycoms,
                            const void* pi, const void* theta, uint8_t* ok);
int gs_verify_statement(gs_ctx*, int equ_type, size_t E, int m, int n, const void* A, const void* B, const void* Gamma,
                        const void* target, const void* xcoms, const void* ycoms, const void* pi, const void* theta,
                        uint8_t* ok);
/* ---- evaluate: what an equation evaluates to at a witness, and whether a witness satisfies it -----------------------
 * Every equation carries a target; a statement builder computes it from the witness before anything can be proved, and a
 * prover wants to know that its witness satisfies the equation BEFORE it pays for a proof that the verifier rejects
 * (Provable::prove does not check).  Layouts are those of gs_prove_batch / gs_verify_batch: X[N][m], Y[N][n], A[N][n],
 * B[N][m], Gamma[N][m][n], target[N], ok[N]; the _statement forms take ONE copy of X[m], Y[n] for all E equations, exactly
 * as gs_prove_statement does.  The value of equation e (the left-hand sides of src/statement.rs:17-21):
 *   GS_PPE    : prod_j e(A_j, Y_j) * prod_i e(X_i, B_i) * prod_ij e(X_i, Y_j)^Gamma_ij   a canonical GT element in boundary
 *               form: for the same pairs the bytes gs_multi_pairing_batch writes, and what a verifying PPE target equals
 *   GS_MSMEG1 : sum_j y_j A_j + sum_i b_i X_i + sum_ij Gamma_ij y_j X_i   normalised affine G1, the identity all-zero bytes
 *   GS_MSMEG2 : sum_j a_j Y_j + sum_i x_i B_i + sum_ij Gamma_ij x_i Y_j   the same in G2
 *   GS_QUAD   : sum_j a_j y_j + sum_i x_i b_i + sum_ij x_i Gamma_ij y_j   a canonical Montgomery Fr
 * gs_eval_*: target_out[e] = that value.  gs_check_witness_*: ok[e] = 1 iff the value of equation e equals target[e] AS AN
 * ELEMENT; the comparison is on the boundary limbs of the canonical value, so a target with non-canonical limbs never
 * matches.
 * How it is computed: the Gamma term is FOLDED so that it costs no pairing and no scalar multiplication
 * of its own -- PPE: W_j = A_j + sum_i Gamma_ij X_i in G1 (n short sums over the same m bases), then m + n Miller pairs
 * and ONE final exponentiation per equation (a 4 x 4 PPE: 8 pairs and one, where gs_verify_batch pays 40 and four); MSMEG1 / MSMEG2:
 * one sum of m + n terms with the scalars c_i = b_i + sum_j Gamma_ij y_j (d_j = a_j + sum_i x_i Gamma_ij) folded in Fr;
 * QuadEqu: one lane of Fr arithmetic per equation.
 * A CRS must be installed (GS_ERR_NOCRS) although none of its elements is read.  Shapes and errors as gs_prove_batch;
 * N == 0 is a no-op.  The host forms return GS_ERR_ARG when the output overlaps an input; for the _dev forms that is the
 * caller's contract.  The _dev forms only enqueue on the context's stream.  The calls are refused inside a mixed call
 * (GS_ERR_ARG).  The multi-GPU handles (gs_multi_*) have NO counterpart: use a shard's context (gs_multi_ctx).  Points
 * outside the prime-order subgroups fall under the rule at the top of this file; "endo" = 0 is followed (the variable-base
 * lanes run plain, "k_var.plain").  "var_tm", "var_mo", "var_w", "var_w2", "var_ws_lanes", "red_k", "miller_ch" and
 * "coop_fe" act as they do elsewhere, "var_tab" = 1 puts the PPE's W_j on shared window tables of the X_i; "line_tables"
 * has nothing to act on: no argument is a CRS element, every line is stepped.
 * WHEN TO CALL IT (tools/eval_rate.py, profiles/eval/rate.json, DESIGN.md 6.8: BLS12-381, 4 x 4, one MI355X, device-
 * resident, median of 7, entries alternating), ms per call at N = 2^12 / 2^14 / 2^16 -- PPE: this entry 14.4 / 23.2 / 62.1,
 * gs_verify_batch_dev on the same batch 20.6 / 55.5 / 197.4, gs_prove_batch_dev 8.4 / 19.6 / 64.9, gs_multi_pairing_batch_dev
 * on 8 arbitrary pairs per row (no Gamma work) 42.3 / 43.0 / 48.5; BN254 PPE at 2^16: 44.2 against 143.9 (verify); MSMEG1:
 * 1.9 / 2.8 / 8.3 against 19.7 / 49.4 / 185.4 (verify).  gs_check_witness_* costs what gs_eval_* costs.  Call
 * gs_check_witness_* before gs_prove_batch whenever the witness is not known to be good: at 2^16 it costs 0.24 of the
 * prove + verify a bad witness would waste (PPE; 0.04 for MSMEG1) and names the failing equations.  For targets, call
 * gs_eval_* rather than pairing the Gamma term out by hand: below ~2^15 rows it is also faster than gs_multi_pairing_batch on
 * the m + n pairs alone (that entry runs one lane per row), above it it costs the Gamma sum more (13.5 of 62.1 ms at 2^16).
 * Kernel profile names: "k_prep_eval[.a]", "k_fix.ev1" (the PPE's addends A_j), "k_var*.ev1|.ev2", "k_red.ev1|.ev2",
 * "k_miller.eval" (gs_prof_get_work: pairs), "k_cell_fold", "k_final_eval[.coop]", "k_eval_cmp" (the point types' check). */
int gs_eval_batch_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                      const void* B, const void* Gamma, void* target_out);
int gs_eval_batch(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                  const void* B, const void* Gamma, void* target_out);
int gs_eval_statement_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                          const void* B, const void* Gamma, void* target_out);
int gs_eval_statement(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                      const void* B, const void* Gamma, void* target_out);
int gs_check_witness_batch_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                               const void* B, const void* Gamma, const void* target, uint8_t* ok);
int gs_check_witness_batch(gs_ctx*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                           const void* B, const void* Gamma, const void* target, uint8_t* ok);
int gs_check_witness_statement_dev(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y,
                                   const void* A, const void* B, const void* Gamma, const void* target, uint8_t* ok);
int gs_check_witness_statement(gs_ctx*, int equ_type, size_t E, int m, int n, const void* X, const void* Y, const void* A,
                               const void* B, const void* Gamma, const void* target, uint8_t* ok);
/* ---- mixed batches and mixed-type Statements: several sub-batches in ONE call ------------------------------------
 * configs[2] of the baseline mixes PPE, MSMEG1 and MSMEG2 equations; the reference's Statement is a list of equations
 * of ANY type over one list of variables (src/statement.rs:24-28,109).  A part is a homogeneous sub-batch (type, N, m,
 * n and the arrays of gs_prove_batch / gs_verify_batch for it); parts may differ in type AND shape.  Outputs are
 * byte-identical to one gs_prove_batch / gs_verify_batch call per part.  How the parts run ("mixed_merge"):
 *   - up to 2^14 equations per call (16 x the device's SIMDs): RECORD AND MERGE on the context's own stream.  Every part's
 *     launches are recorded (nothing is enqueued; the part's scratch buffers carry a per-part tag so that they are live
 *     side by side), then replayed in step: launches of different parts that run the same kernel body become ONE
 *     segmented launch (k_seg, up to 4 segments), so a mixed batch of a few thousand equations fills the chip like a
 *     homogeneous batch of its total size (2^12: 0.92-0.94 of the PPE-only rate);
 *   - larger calls, a single part, or while the kernel profile is on: the parts run one after the other on the
 *     context's stream, each with its own lane shapes (every part fills the chip by itself from ~2^15 on).
 * There are no child contexts or extra streams (measured and rejected: profiles/r3/mixed_streams.txt).
 * shared_vars != 0 makes the part a Statement's: X, Y, R, S hold ONE copy (m / n entries) that all N equations of the
 * part use, xcoms / ycoms are the statement's commitments (m / n entries; prove writes them when non-NULL -- pass them
 * with ONE of the parts that use a variable group and NULL with the others -- verify reads them), i.e. exactly
 * gs_prove_statement / gs_verify_statement per part.  A mixed-type Statement over G1 variables Xg, G2 variables Yg
 * and scalar variables xs, ys is then one call with the parts PPE (Xg, Yg), MSMEG1 (Xg, ys), MSMEG2 (xs, Yg) and
 * QuadEqu (xs, ys) pointing at the shared groups.  At most GS_MIXED_MAX parts per call. */
#define GS_MIXED_MAX 8
typedef struct {
  int equ_type;
  size_t N;
  int m, n;
  const void *X, *Y, *A, *B, *Gamma, *R, *S, *T;
  void *xcoms, *ycoms, *pi, *theta;
  int shared_vars;
} gs_prove_part;
typedef struct {
  int equ_type;
  size_t N;
  int m, n;
  const void *A, *B, *Gamma, *target, *xcoms, *ycoms, *pi, *theta;
  uint8_t* ok;
  int shared_vars;
} gs_verify_part;
int gs_prove_mixed_dev(gs_ctx*, int nparts, const gs_prove_part* parts);
int gs_prove_mixed(gs_ctx*, int nparts, const gs_prove_part* parts);
int gs_verify_mixed_dev(gs_ctx*, int nparts, const gs_verify_part* parts);
int gs_verify_mixed(gs_ctx*, int nparts, const gs_verify_part* parts);

/* Batched pairing-product check: random linear combination of all 4N cell
 * equations with caller-supplied 64-bit exponents rho[N][4] (device/host u64).
 * RHO CONTRACT (soundness rests on it): every rho is drawn from a CSPRNG, fresh for every call, NON-ZERO, secret
 * until the verdict is out, and drawn AFTER the commitments and proofs of the batch are fixed.  A predictable or
 * reused rho lets a prover craft a batch that passes the combined check while single equations fail; the soundness
 * error is 2^-64 per batch for honest-size exponents.  The host entry rejects rho == 0 (GS_ERR_ARG); the _dev entry
 * cannot look.  PPE targets are raised to rho WITHOUT a subgroup check: a target outside the order-r subgroup of GT
 * (impossible for a decoded, validated PairingOutput, gs_wire_decode_gt validate = 1) is the caller's to exclude.
 * The exact entry points above have no such contract.
 * one final exponentiation for the whole batch.  *ok_all = 1 iff the combined
 * check passes; acc (may be NULL for the host entry) receives the accumulator PAIR
 * (2 GT): acc[0] = prod Miller(e,cell)^rho (un-exponentiated), acc[1] = prod t_e^rho
 * (1 for the non-PPE types).  acc[0] is defined up to factors the final exponentiation removes: its BYTES are a
 * function of the inputs and of "line_tables" (tabulated and stepped lines differ by elements of a proper subfield),
 * never of what the context did before; acc[1] and the verdict follow no option.  Ranks exchange their pairs (all-gather) and
 * gs_gt_finalize(count, pairs) multiplies them in the given order and checks
 * FE(prod acc[0]) == prod acc[1]: the verdict for the union of the batches. */
int gs_verify_batch_rlc_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                            const void* Gamma, const void* target, const void* xcoms, const void* ycoms,
                            const void* pi, const void* theta, const uint64_t* rho, void* acc_gt);
int gs_verify_batch_rlc(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                        const void* Gamma, const void* target, const void* xcoms, const void* ycoms, const void* pi,
                        const void* theta, const uint64_t* rho, void* acc_gt, uint8_t* ok_all);
/* The batched check WITH FAULT LOCALISATION: the same inputs, layouts and accumulator pair as gs_verify_batch_rlc, and
 * one byte per equation that says where the faults are.  The products of gs_verify_batch_rlc are taken as a K-ary tree
 * (K = 8, "locate_k") whose levels are KEPT in device memory:
 *   leaf e            (f_e, t_e): f_e = the product of equation e's Miller partials, t_e = target_e^rho[e][3] for PPE,
 *                     one otherwise
 *   node (l, i)       the product of its at most K children (l - 1, i K .. i K + K - 1); the root is the pair acc_gt
 *   a node PASSES     iff FE(f) == t
 * and descended: the root is checked; every child of a failing node is checked, down to the leaves (no child is inferred
 * from its siblings).
 *   ok[e] = 0         iff leaf e was reached and failed
 *   ok[e] = 1         iff e lies under some node that passed (the root included).  This is NOT exact verification: a set
 *                     of faults that cancels inside a passing node is not seen -- nor does gs_verify_batch_rlc see it.
 *   info[0]           the number of entries with ok == 0
 *   info[1]           the number of node checks (final exponentiations) of the descent: 1 for the root plus, for every
 *                     failing internal node, the number of its children.  Both are functions of the inputs and K alone.
 *   acc_gt            the root pair, byte for byte what gs_verify_batch_rlc_dev writes for the same inputs and options.
 * RHO CONTRACT: that of gs_verify_batch_rlc above, unchanged (CSPRNG, fresh per call, NON-ZERO, secret until the
 * verdicts are out, drawn after the batch is fixed; PPE targets are raised to rho without a subgroup check).  Every node
 * check is a random linear combination over that node's leaves with the SAME exponents, so the soundness error of a
 * call is at most info[1] * 2^-64.
 * Cost: a valid batch costs what gs_verify_batch_rlc costs (one node check); b bad proofs cost about b K log_K N more
 * final exponentiations, against the 4 N of gs_verify_batch.  Advice to callers, from the measurement of DESIGN.md 6.6
 * (2^16 PPE 4 x 4, one MI355X): there is NO crossover -- the descent is a chain of one-level launches, about 30 ms from one
 * bad proof to all 65536 of them, for scattered and for contiguous faults alike, so combined check plus descent (186 ..
 * 189 ms) stays below one exact pass (202 ms) even when every proof is bad, and a valid batch costs the combined check
 * alone (157.9 against 157.7 ms).  Call this entry instead of gs_verify_batch_rlc followed by gs_verify_batch; call
 * gs_verify_batch when the verdicts must be exact (see ok[e] = 1 above).
 * Memory: the stored levels take about 2 N K / (K - 1) GT elements for PPE and half that otherwise, next to the
 * N * ntask Miller partials gs_verify_batch_rlc keeps anyway.
 * The _dev entry only enqueues on the context's stream (the frontier of failing nodes and its length stay in device
 * memory; every level's launch is sized for the whole level); ok[N], info[2] and acc_gt are device pointers, all
 * required.  The host entry stages like the other host entries, rejects rho == 0 and outputs that overlap an input or
 * each other (GS_ERR_ARG), and returns when ok, info and acc_gt are back; acc_gt and info may be NULL there.  N == 0 is
 * GS_ERR_ARG; N >= 2^29 is GS_ERR_SHAPE (node indices and the items of a level's launch are 32-bit).  "endo" 0 is
 * followed as in gs_verify_batch_rlc; "coop_fe" selects the one-lane or the 3-lane final exponentiation of the node
 * checks (0 / 2 force, 1 plans per level from the launch size).  The multi-GPU handles (gs_multi_*) have no counterpart.
 * Kernel profile names: "k_rlc_leaf", "k_rlc_tree" (one launch per level), "k_rlc_locate[.coop]" (one launch per level). */
int gs_verify_batch_rlc_locate_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                                   const void* Gamma, const void* target, const void* xcoms, const void* ycoms,
                                   const void* pi, const void* theta, const uint64_t* rho, void* acc_gt,
                                   uint8_t* ok /* [N] */, uint32_t* info /* [2] */);
int gs_verify_batch_rlc_locate(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                               const void* Gamma, const void* target, const void* xcoms, const void* ycoms,
                               const void* pi, const void* theta, const uint64_t* rho, void* acc_gt,
                               uint8_t* ok /* [N] */, uint32_t* info /* [2] */);
/* Batched verifier for STATEMENTS: S statements of one type and shape, each E equations over ONE set of commitments
 * (the arrays of statement s are exactly what gs_verify_statement takes, at offset s: A[S][E][n], B[S][E][m],
 * Gamma[S][E][m][n], target[S][E], xcoms[S][m], ycoms[S][n], pi[S][E][kx], theta[S][E][ky]; rho[S][E][4] u64).
 * The random linear combination is taken ACROSS the equations of a statement before anything is paired, so a
 * statement costs 2n + 2m + 2kx + 2ky Miller pairs (fewer with scalar constants) whatever E is; the E-dependent work
 * is short-scalar sums in G1 / G2.  One verdict per statement: ok[S].
 * acc_gt[S][2] (may be NULL for the host entry) receives one accumulator pair per statement in the convention of
 * gs_verify_batch_rlc: acc[s][0] = the un-exponentiated Miller product, FE(acc[s][0]) = prod_e prod_cells
 * (lhs / rhs without the PPE target)^rho_e,cell; acc[s][1] = prod_e t_e^rho_e,11 for PPE, one otherwise;
 * ok[s] = (FE(acc[s][0]) == acc[s][1]).
 * RHO CONTRACT (soundness rests on it), as for gs_verify_batch_rlc: every rho is drawn from a CSPRNG, fresh for every
 * call, NON-ZERO, secret until the verdict is out, and drawn AFTER the commitments and proofs are fixed; the soundness
 * error is 2^-64 per statement.  The host entry rejects rho == 0 (GS_ERR_ARG); the _dev entry cannot look.  PPE targets
 * are raised to rho WITHOUT a subgroup check.
 * A statement that mixes equation types is checked with one call per type (S = 1) and the pairs handed to
 * gs_gt_finalize: the verdict of the whole statement.  S = 0 or E = 0 is GS_ERR_ARG; a statement whose arrays the
 * plan cannot index (32-bit byte strides per statement) is GS_ERR_SHAPE. */
int gs_verify_statements_rlc_dev(gs_ctx*, int equ_type, size_t S, size_t E, int m, int n, const void* A, const void* B,
                                 const void* Gamma, const void* target, const void* xcoms, const void* ycoms,
                                 const void* pi, const void* theta, const uint64_t* rho, void* acc_gt, uint8_t* ok);
int gs_verify_statements_rlc(gs_ctx*, int equ_type, size_t S, size_t E, int m, int n, const void* A, const void* B,
                             const void* Gamma, const void* target, const void* xcoms, const void* ycoms, const void* pi,
                             const void* theta, const uint64_t* rho, void* acc_gt, uint8_t* ok);
/* Batched verifier for N PROOFS OF ONE EQUATION: the public equation (A[n], B[m], Gamma[m][n], target[1]) exists ONCE,
 * every proof e brings its own xcoms[N][m], ycoms[N][n], pi[N][kx], theta[N][ky]; rho[N][4] u64 as above.  This is the
 * traffic gs_rerandomize_batch produces (re-shown credentials, ballots, mix-net outputs).  Because the constants are
 * shared, the random linear combination is taken ACROSS the proofs before pairing wherever the other argument of a pair
 * is a constant or a CRS element: per proof only the Gamma term is paired, 2n pairs (plus 2kx for pi
 * unless "eq_pi" = 1); m (or 2) + 2ky (+ 2kx) pairs and ONE target power t^(sum_e rho_e,11) are paid per call.  The
 * price is a K-ary sum of N points per folded term.
 * All four equation types, both curves, shapes as everywhere else.  acc_gt[2] (may be NULL for the host entry) receives
 * the accumulator pair in the convention of gs_verify_batch_rlc, so that pairs of several calls or ranks combine through
 * gs_gt_finalize: FE(acc[0]) = prod_e prod_cells (lhs / rhs without the PPE target)^rho_e,cell (acc[0] itself is an
 * un-exponentiated value: only its FE is defined); acc[1] = t^(sum_e rho_e,11) for PPE, one otherwise, a canonical GT
 * element: byte for byte what gs_verify_batch_rlc writes for the same proofs with the constants replicated N times.
 * *ok_all (host entry, may be NULL) = 1 iff FE(acc[0]) == acc[1].
 * RHO CONTRACT (soundness rests on it), that of gs_verify_batch_rlc: every rho is drawn from a CSPRNG, fresh for every
 * call, NON-ZERO, secret until the verdict is out, and drawn AFTER the commitments and proofs of the batch are fixed.
 * A predictable or reused rho lets a prover craft a batch that passes the combined check while single proofs fail; the
 * soundness error is 2^-64 per call.  The host entry rejects rho == 0 (GS_ERR_ARG); the _dev entry cannot look.  The
 * PPE target is raised WITHOUT a subgroup check.
 * The host entry stages the four constant arrays once (one copy each) and the four per-proof arrays.  N == 0 is
 * GS_ERR_ARG; N >= 2^32 is GS_ERR_SHAPE; the entry is refused inside a mixed call (GS_ERR_ARG).  "endo" 0 is followed
 * as in gs_verify_batch_rlc; "miller_ch" and "line_tables" act as there, "var_tm" forces the terms per Straus lane of
 * its passes.  The multi-GPU handles (gs_multi_*) have NO counterpart, and there is no fault localisation: a failing
 * batch goes to gs_verify_batch_rlc_locate with the constants replicated.
 * WHEN TO CALL IT (tools/eq_rlc_rate.py, profiles/eq_rlc/rate.json, DESIGN.md 6.7: BLS12-381, 4 x 4, one MI355X, device-
 * resident, median of 7, entries alternating): time of gs_verify_batch_rlc on replicated constants over the time of this
 * entry at N = 2^12 / 2^14 / 2^16 -- PPE 1.06 / 1.03 / 1.32; QuadEqu 0.77 / 0.98 / 1.16.  A ratio below 1 means
 * gs_verify_batch_rlc is the faster entry at that size: PPE: at or above parity from 2^12 on; QuadEqu: crossover
 * between 2^14 and 2^16 (0.98 at 2^14 is inside the spread of that run: treat 2^14 as parity).
 * Below the crossover call gs_verify_batch_rlc unless replicating the constants is what hurts; above it call this entry.
 * Kernel profile names: "k_prep_verify_eq_rlc[.shared]", "k_batch_sum.eqs1|.eqs2", "k_miller.eqrlc" (the per-proof
 * pairs), "k_miller.eqrlc.batch" (the pairs paid once), "k_eq_rlc_tpow". */
int gs_verify_equation_rlc_dev(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A /* [n] */,
                               const void* B /* [m] */, const void* Gamma /* [m][n] */, const void* target /* [1] */,
                               const void* xcoms /* [N][m] */, const void* ycoms /* [N][n] */, const void* pi /* [N][kx] */,
                               const void* theta /* [N][ky] */, const uint64_t* rho /* [N][4] */, void* acc_gt /* [2] */);
int gs_verify_equation_rlc(gs_ctx*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                           const void* Gamma, const void* target, const void* xcoms, const void* ycoms, const void* pi,
                           const void* theta, const uint64_t* rho, void* acc_gt /* may be NULL */, uint8_t* ok_all);
/* product of `count` GT accumulator pairs (host), final exponentiation, FE(prod acc[0]) == prod acc[1] ? */
int gs_gt_finalize(gs_ctx*, size_t count, const void* accs_gt_host, uint8_t* ok_all);
/* the same with the pairs in this context's device memory (e.g. the receive buffer of an all-gather); ok_all on the host */
int gs_gt_finalize_dev(gs_ctx*, size_t count, const void* accs_gt_dev, uint8_t* ok_all);

/* ---- several GPUs of one node ----------------------------------------------------------
 * gs_ctx_create_multi owns one SHARD per listed device ordinal: a context (stream, scratch; CRS tables shared per
 * device) and a persistent host thread bound to that device.  A batch is cut into contiguous blocks of equation
 * indices, block i on shard i (sizes differ by at most one: gs_multi_shard); every block runs the single-device entry
 * point of the same name on its shard's thread.  Identical bytes to a single-device run.  Prove and exact verify use
 * no collective.  The batched verifier's per-shard accumulator pairs (2 GT each) are written into per-shard exchange
 * buffers on their devices, all-gathered (RCCL over xGMI when the shards sit on distinct devices; device-to-device /
 * peer copies for one shard, shards sharing a device or a missing librccl: gs_multi_exchange_note says which),
 * cross-checked, multiplied in shard order on device 0 and finished with ONE final exponentiation: the verdict for the
 * union of the blocks (same rho contract as gs_verify_batch_rlc; rho is indexed by GLOBAL equation number).
 * acc_pairs (host, may be NULL) receives the ndev gathered pairs.  RCCL is bound at run time (dlopen of librccl.so,
 * preferring a copy already in the process).
 *   host-pointer family: whole batch in, whole batch out; every shard stages its block through its context's pinned
 *     pipeline (see gs_prove_batch).
 *   _dev family: arrays of ndev DEVICE pointers, entry i = shard i's block already resident on devices[i] (what a
 *     caller that produced the data on the GPUs holds); nothing crosses PCIe; calls return once every shard has
 *     enqueued its kernels, gs_multi_sync joins.  (gs_multi_verify_batch_rlc_dev returns the verdict, so it joins.)
 * GS_MULTI_SHARED_DEVICES lets several shards name the SAME ordinal: the split, offsets, empty blocks and the pair
 * exchange then run on one GPU exactly as they would on eight (how tests exercise ndev > 1 on a one-GPU box). */
typedef struct gs_multi gs_multi;
enum { GS_MULTI_SHARED_DEVICES = 1 };
int gs_ctx_create_multi(int curve_id, const int* device_ordinals, int ndev, gs_multi** out);
int gs_ctx_create_multi_ex(int curve_id, const int* device_ordinals, int ndev, int flags, gs_multi** out);
void gs_multi_destroy(gs_multi*);
int gs_multi_ndev(gs_multi*);
gs_ctx* gs_multi_ctx(gs_multi*, int i);                      /* shard i's context, e.g. for gs_set_option */
const char* gs_multi_last_error(gs_multi*);
int gs_multi_uses_rccl(gs_multi*);                           /* 1 once the RCCL communicators exist */
const char* gs_multi_exchange_note(gs_multi*);               /* how the accumulator pairs travel (and why not RCCL) */
/* The pair exchange walks three legs -- 0 RCCL all-gather, 1 device / peer copies (hipMemcpyPeerAsync; peer access is
 * probed and enabled at gs_ctx_create_multi), 2 host-staged copies -- and a leg that FAILS AT RUN TIME is marked failed
 * and the same call retries on the next one (it is not an error while a slower way exists; gs_multi_exchange_note names
 * the leg used and why earlier ones failed).  Options: "exchange_leg" 0..2 start the chain there; "exchange_fail" bit
 * mask: leg k fails when it runs (test hook: how the chain is exercised on a one-GPU box; also GS_MULTI_EXCHANGE_FAIL /
 * GS_MULTI_EXCHANGE_LEG at create); "exchange_reset": forget earlier failures. */
int gs_multi_set_option(gs_multi*, const char* key, int value);
int gs_multi_shard(gs_multi*, size_t N, int i, size_t* lo, size_t* hi); /* block [lo, hi) of shard i */
int gs_multi_set_crs(gs_multi*, const void* crs_host);
int gs_multi_sync(gs_multi*);                                /* drain every shard's stream */
int gs_multi_prove_batch(gs_multi*, int equ_type, size_t N, int m, int n, const void* X, const void* Y, const void* A,
                         const void* B, const void* Gamma, const void* R, const void* S, const void* T, void* xcoms,
                         void* ycoms, void* pi, void* theta);
int gs_multi_verify_batch(gs_multi*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                          const void* Gamma, const void* target, const void* xcoms, const void* ycoms, const void* pi,
                          const void* theta, uint8_t* ok);
int gs_multi_verify_batch_rlc(gs_multi*, int equ_type, size_t N, int m, int n, const void* A, const void* B,
                              const void* Gamma, const void* target, const void* xcoms, const void* ycoms,
                              const void* pi, const void* theta, const uint64_t* rho, void* acc_pairs_gt,
                              uint8_t* ok_all);
int gs_multi_prove_batch_dev(gs_multi*, int equ_type, size_t N, int m, int n, const void* const* X,
                             const void* const* Y, const void* const* A, const void* const* B,
                             const void* const* Gamma, const void* const* R, const void* const* S,
                             const void* const* T, void* const* xcoms, void* const* ycoms, void* const* pi,
                             void* const* theta);
int gs_multi_verify_batch_dev(gs_multi*, int equ_type, size_t N, int m, int n, const void* const* A,
                              const void* const* B, const void* const* Gamma, const void* const* target,
                              const void* const* xcoms, const void* const* ycoms, const void* const* pi,
                              const void* const* theta, uint8_t* const* ok);
/* rho[i]: shard i's exponents on its device, 4 per equation of ITS block */
int gs_multi_verify_batch_rlc_dev(gs_multi*, int equ_type, size_t N, int m, int n, const void* const* A,
                                  const void* const* B, const void* const* Gamma, const void* const* target,
                                  const void* const* xcoms, const void* const* ycoms, const void* const* pi,
                                  const void* const* theta, const uint64_t* const* rho, void* acc_pairs_gt_host,
                                  uint8_t* ok_all);

/* ---- L2 parity hooks (host pointers) ------------------------------------- */
/* out[i] = sum_k lhs[i][k] * col[k]       (data_structures.rs:696-742) */
int gs_mat_left_mul_com1(gs_ctx*, int rows, int k, const void* lhs_fr, const void* col_com1, void* out_com1);
int gs_mat_left_mul_com2(gs_ctx*, int rows, int k, const void* lhs_fr, const void* col_com2, void* out_com2);
/* ComT::pairing_sum(x[0..k), y[0..k)) -> 4 GT cells (00,01,10,11)   (data_structures.rs:494-502) */
int gs_pairing_sum(gs_ctx*, int k, const void* x_com1, const void* y_com2, void* out_comt);
/* Matrix<Fr> product out = lhs (rows x inner) * rhs (inner x cols), row-major Montgomery Fr, host pointers, computed by
 * the prover's scalar-preparation kernels (Psi = R^T Gamma, prove.rs:133): the reference's Mat::right_mul / left_mul on
 * Matrix<Fr> (data_structures.rs:824-912) and the hook its matrix KATs (:1726-1947) run through. */
int gs_fr_matmul(gs_ctx*, int rows, int inner, int cols, const void* lhs_fr, const void* rhs_fr, void* out_fr);
/* batch helpers: out[i] = k[i] * P[i] (P broadcast if p_stride == 0), E::multi_pairing per row */
int gs_g1_mul_batch(gs_ctx*, size_t count, const void* p_g1, int p_broadcast, const void* k_fr, void* out_g1);
int gs_g2_mul_batch(gs_ctx*, size_t count, const void* p_g2, int p_broadcast, const void* k_fr, void* out_g2);
int gs_g1_mul_batch_dev(gs_ctx*, size_t count, const void* p_g1, int p_broadcast, const void* k_fr, void* out_g1);
int gs_g2_mul_batch_dev(gs_ctx*, size_t count, const void* p_g2, int p_broadcast, const void* k_fr, void* out_g2);
int gs_multi_pairing_batch(gs_ctx*, size_t count, int k, const void* p_g1, const void* q_g2, void* out_gt);
int gs_multi_pairing_batch_dev(gs_ctx*, size_t count, int k, const void* p_g1, const void* q_g2, void* out_gt);
/* out[i] = base^(k[i]) in GT (k canonical-Montgomery Fr); used to synthesise satisfied PPE targets */
int gs_gt_pow_batch_dev(gs_ctx*, size_t count, const void* base_gt_dev, const void* k_fr, void* out_gt);

/* ---- canonical wire format (ark-serialize) -----------------------------------
 * Arrays of elements between the boundary form above and the byte strings ark-serialize produces for
 * the reference's derives (src/data_structures.rs:128,132 Com1/Com2; src/prover/commit.rs:18,24;
 * src/prover/prove.rs:55; src/statement.rs:117-179; src/generator.rs:35): Fr / Fq little-endian canonical
 * integers; GT = 12 Fq; BLS12-381 points in ark-bls12-381's zcash-compatible big-endian flagged form,
 * BN254 points in ark-ec's default little-endian flagged form (details: csrc/gs_wire.cuh).  Struct
 * framing (Vec<T> = u64-LE length + items, fields in declaration order, EquType = 1 byte) is host-side:
 * include/gs_amd.hpp, groth_sahai_rs_amd/wire.py.  Host pointers.  decode: ok[i] = 1 iff element i is a
 * well-formed encoding (canonical coordinates, consistent flags, on the curve) and, with validate != 0,
 * passes the r-torsion check of ark-serialize's Validate::Yes; rejected elements decode to the identity
 * (points) / zero (Fr; GT: all twelve coefficients).  Every element has exactly ONE accepted encoding per form.  The
 * identity is the infinity flag, an all-zero payload and no sort flag: ark-bls12-381 ignores the payload once it sees the
 * infinity flag, this decoder does not.  A BN254 uncompressed point carries the sort flag of its y: ark-ec ignores that
 * flag next to an explicit y, this decoder does not.  (Stricter in both; arkworks' own serialiser never produces the other
 * byte strings.)  sizes: out[0..5] = G1 compressed, G1 uncompressed, G2 compressed, G2 uncompressed, Fr, GT. */
int gs_wire_sizes(int curve_id, size_t out[6]);
int gs_wire_encode_g1(gs_ctx*, size_t n, int compressed, const void* pts_g1, uint8_t* out);
int gs_wire_encode_g2(gs_ctx*, size_t n, int compressed, const void* pts_g2, uint8_t* out);
int gs_wire_decode_g1(gs_ctx*, size_t n, int compressed, int validate, const uint8_t* in, void* pts_g1, uint8_t* ok);
int gs_wire_decode_g2(gs_ctx*, size_t n, int compressed, int validate, const uint8_t* in, void* pts_g2, uint8_t* ok);
int gs_wire_encode_fr(gs_ctx*, size_t n, const void* fr, uint8_t* out);
int gs_wire_decode_fr(gs_ctx*, size_t n, const uint8_t* in, void* fr, uint8_t* ok);
int gs_wire_encode_gt(gs_ctx*, size_t n, const void* gt, uint8_t* out);
int gs_wire_decode_gt(gs_ctx*, size_t n, int validate, const uint8_t* in, void* gt, uint8_t* ok);

/* ---- subgroup safety for in-memory points (the wire decoder's tests without the wire format) ----------------------
 * ok[i] = 1 iff point i of pts (G1: group = 1, G2: group = 2; boundary limbs as everywhere) has canonical coordinates
 * (every word string < p), is the identity (0, 0) or lies on the curve, AND is in the prime-order subgroup (BLS12-381:
 * the endomorphism tests arkworks uses; BN254 G1: cofactor 1, G2: [r]Q = O).  The reference needs no such call: its
 * double-and-add takes any curve point (src/data_structures.rs:336-342) and arkworks' deserialisation has validated
 * everything it holds. */
int gs_validate_points_dev(gs_ctx*, int group, size_t n, const void* pts_dev, uint8_t* ok_dev);
int gs_validate_points(gs_ctx*, int group, size_t n, const void* pts, uint8_t* ok);

/* ---- measurement hook ----------------------------------------------------
 * Name and average duration (ms, HIP events on the context's stream) of the
 * kernels launched since gs_prof_reset; used by bench.py for the roofline. */
int gs_prof_enable(gs_ctx*, int on);
int gs_prof_reset(gs_ctx*);
int gs_prof_get(gs_ctx*, int idx, char* name, size_t name_cap, double* total_ms, uint64_t* launches);
/* lane-tasks launched under that name and its kernel-specific work items (fixed-base scalars for k_fix, terms for
 * k_var_multi, partial sums for k_red, pairs for k_miller, lanes otherwise): inputs of bench.py's ALU roofline */
int gs_prof_get_work(gs_ctx*, int idx, uint64_t* lanes, uint64_t* work);
/* the clock (GHz) the launches under entry idx ran at, measured INSIDE them: every wave of a segmented launch stamps
 * s_memtime (shader cycles) and s_memrealtime (100 MHz) around its body while the profile is on; 0 where unavailable.
 * bench.py prices the multiply-add issue peak at this clock (one measurement: no separate clock correction). */
int gs_prof_get_clock(gs_ctx*, int idx, double* ghz);

#ifdef __cplusplus
}
#endif
#endif /* GS_AMD_H */
