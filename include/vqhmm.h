/* vqhmm — C-ABI of the MI355X-native VAE_HMM hot path (libvqhmm.so, gfx950).
 *
 * The reference (yashnaray/VQ-VAE-HMM-model) is pure Python/PyTorch and exposes
 * no FFI: its boundary is the nn.Module surface of VQ_VAE_HMM_fixed.py.  Each
 * entry point below replaces the ATen work behind one piece of that surface
 * (citations per function).  The Python package `vqhmm` binds these with
 * ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (allocated by the caller, e.g. the
 *    PyTorch caching allocator) unless documented otherwise; the library never
 *    allocates, frees or synchronises.  Scratch memory is a caller-provided
 *    workspace whose size comes from the matching *_workspace_size query.
 *  - Work is enqueued on `stream` (a hipStream_t; NULL = default stream) and
 *    is asynchronous; kernel faults surface at the caller's next sync.
 *  - Return value: 0 on success, negative VQHMM_E* code on bad arguments or a
 *    failed launch.  No global mutable state: calls are reentrant from any
 *    host thread with its own stream, and graph-capturable.
 *  - Tensors are dense row-major in the reference's layouts: "CF" = (B, C, T)
 *    channels-first as nn.Conv1d uses; log_A is (B, T, K, K) with index t the
 *    transition t-1 -> t (VQ_VAE_HMM_fixed.py:69,125-127).
 *  - fp32 throughout (the reference computes in fp32).
 */
#ifndef VQHMM_H
#define VQHMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQHMM_OK 0
#define VQHMM_EINVAL -1
#define VQHMM_ELAUNCH -2
#define VQHMM_EWORKSPACE -3
#define VQHMM_EUNSUPPORTED -4

/* Bits of the training step's device status word (vqhmm_elbo_status_offset).  Kernels only
 * ever OR bits in; the caller zeroes the word when it allocates the workspace and reads it
 * after a synchronisation (TrainState.check_status raises RuntimeError on any bit). */
#define VQHMM_STATUS_TAIL_TIMEOUT 1ull /* reserved: no kernel sets it (no launch waits on another
                                          * workgroup); kept so callers' status checks stay valid */

/* Number of parameter tensors of a VAE_HMM, in nn.Module.parameters() order
 * (VQ_VAE_HMM_fixed.py:92-98 -> encoder :32-36, prior :44-57, decoder :74-79). */
#define VQHMM_NPARAMS 18

/* Constructor arguments of VAE_HMM(input_dim, hidden_dim, K, hidden_dim2,
 * u_dim, trans_hidden)  (VQ_VAE_HMM_fixed.py:93). */
typedef struct vqhmm_dims {
  int32_t input_dim;    /* D  */
  int32_t hidden_dim;   /* H  (encoder conv1, decoder embedding + convs) */
  int32_t K;            /* number of regimes */
  int32_t hidden_dim2;  /* H2 (encoder conv2) */
  int32_t u_dim;        /* U  */
  int32_t trans_hidden; /* TH */
} vqhmm_dims_t;

/* Library ABI version (bumped on any signature change). */
int32_t vqhmm_abi_version(void);

/* Element offsets of the 18 parameters inside one flat fp32 buffer laid out
 * in parameters() order; offsets[18] = total element count.  Host-only. */
int vqhmm_param_layout(const vqhmm_dims_t* dims, int64_t offsets[VQHMM_NPARAMS + 1]);

/* ---------------------------------------------------------------- VQ ----
 * Nearest-codeword quantization (semantics pseudocode.txt:11
 * `quantize`, hard regimes backtesting.py:154-155 — no reference code).
 * z (B, Dv, T) CF, codebook (K, Dv) -> idx (B, T) int32, dmin (B, T) fp32
 * (nullable).  Expansion form ||z||^2 + ||c_k||^2 - 2 z.c_k, evaluated as
 * s_k = fmaf chain over d ascending of z_d * (-2 c_kd) starting from
 * ||c_k||^2 (itself the fmaf chain of c_kd^2); idx = first k with the
 * smallest s_k; dmin = s_idx + ((q0 + q1) + (q2 + q3)), q_r the fmaf chain of
 * z_d^2 over d = r (mod 4).  Bit-exact vs oracle/c/hmm_oracle.c, non-finite z
 * included (a NaN score is never the minimum; where the oracle's dmin is NaN so
 * is this one).  The inputs z and codebook (of this entry and of
 * vqhmm_vq_quantize_f32) need only 4-byte alignment and give the same idx, dmin
 * and z_q_st bits as 16-byte aligned ones (sse then within 1e-6 relative: another
 * partial-sum order); the outputs and the workspace must be 16-byte aligned. */
int vqhmm_vq_argmin_f32(const float* z, int64_t B, int64_t Dv, int64_t T,
                        const float* codebook, int64_t K,
                        int32_t* idx, float* dmin, void* stream);


/* VQ-VAE quantizer (pseudocode.txt:12-18: `z_q, idx = quantize(z_e, codebook)`, the
 * straight-through z_e + (z_q - z_e).detach() of :13 and the commit / codebook MSEs of :17-18)
 * on channels-first z (B, Dv, T): idx as vqhmm_vq_argmin_f32 (same bit-exact contract),
 * z_q_st[b][d][t] = z + (c[idx][d] - z) in fp32 (the forward value of the straight-through
 * tensor), and *sse = sum over (b, d, t) of (z - c[idx][d])^2 in the direct-difference form,
 * accumulated in fp64 (commit = beta * sse / (B Dv T), codebook loss = sse / (B Dv T)).  Fused in
 * the argmin kernel's epilogue where its row-load path runs (Dv in {4,8,16,32,64}, T % 4 == 0,
 * K <= 32), else argmin + one gather launch; then one fixed-order partial-sum launch (the result
 * is deterministic).  Replaces the reference's `quantize` + two MSEs.
 * Workspace: vqhmm_vq_quantize_workspace_size(B, Dv, T, K) bytes.
 * B * T == 0: VQHMM_OK, *sse = 0 (the empty sum) and nothing else is written. */
size_t vqhmm_vq_quantize_workspace_size(int64_t B, int64_t Dv, int64_t T, int64_t K);
int vqhmm_vq_quantize_f32(const float* z, int64_t B, int64_t Dv, int64_t T, const float* codebook, int64_t K,
                          int32_t* idx, float* z_q_st, double* sse, void* workspace, size_t ws_bytes,
                          void* stream);

/* ------------------------------------------------------------ Viterbi ----
 * MAP state path (semantics math.md:23-67 over Prior.forward's
 * tables VQ_VAE_HMM_fixed.py:59-71 — no reference code).  log_pi (K),
 * log_A (B,T,K,K) [t = transition t-1 -> t], em (B,T,K) emission log-potentials,
 * lengths (B) int64 -> path (B,T) int32 (-1 at t >= length), score (B) fp32.
 * d_t[j] = (max_i d_{t-1}[i] + log_A[t,i,j]) + em[t,j] in fp32, ties -> lowest i;
 * last state = first argmax.  Bit-exact vs oracle/c/hmm_oracle.c.  K <= 4096 (K <= 8: packed lane
 * groups, hmm.hip; 8 < K <= 32: one sequence per wave, hmm_wide.hip; 32 < K <= 4096: one workgroup
 * per sequence, states j, j + 256, .. per thread, 16-bit backpointers past 256 states,
 * hmm_generic.hip); larger K -> VQHMM_EUNSUPPORTED.
 * log_pi, log_A and em need only 4-byte alignment and give the same path and score bits as
 * 16-byte aligned ones (-inf entries included); path, score and the workspace must be 16-byte
 * aligned.
 * Workspace: vqhmm_viterbi_workspace_size(B, T, K) bytes (backpointers as one
 * 64-bit lane ballot per step per wave of 64 / KP^2 sequences, KP = K rounded
 * up to a power of two; T rounded up to 64).
 * T = 0 (or B = 0) returns VQHMM_OK without a launch and writes nothing, score included. */
size_t vqhmm_viterbi_workspace_size(int64_t B, int64_t T, int64_t K);
int vqhmm_viterbi_f32(const float* log_pi, const float* log_A, const float* em, const int64_t* lengths,
                      int64_t B, int64_t T, int64_t K, int32_t* path, float* score, void* workspace,
                      size_t ws_bytes, void* stream);

/* --------------------------------------------------- forward-backward ----
 * Posterior marginals: same inputs as Viterbi ->
 * gamma (B,T,K) fp32 (0 at t >= length), logZ (B) fp32 (NaN if length 0).
 * Base-2 log-space alpha/beta with per-step shifts; a chunk whose fast step
 * leaves float range is recomputed with the max-shifted log-sum-exp.  For
 * 2 <= K <= 8 and 128 <= T <= 1024 (K = 4: T > 256) the kernel is parallel in
 * time (64-step segments' transfer matrices on the matrix cores, a boundary
 * pass, then per-segment chains; hmm_seg.hip); a sequence that leaves the
 * linear range there is recomputed exactly in the same launch.
 * Workspace: vqhmm_fwdbwd_workspace_size(B, T, K) = 2 * B * T * K * 4 bytes.
 * Accuracy target vs the fp64 oracle: |gamma| abs 1e-5, logZ rel 1e-5.  K <= 4096 (as Viterbi).
 * log_pi, log_A and em need only 4-byte alignment: every kernel variant then meets the same
 * accuracy target (K = 4 and K = 8 stage the tables in 16-step instead of 32-step chunks, so the
 * bits may differ from an aligned call's within it); gamma, logZ and the workspace must be 16-byte
 * aligned (the parallel-in-time kernel stores K = 8 gamma rows as 16-byte vectors).
 * T = 0 (or B = 0) returns VQHMM_OK without a launch and writes nothing, logZ included. */
size_t vqhmm_fwdbwd_workspace_size(int64_t B, int64_t T, int64_t K);
int vqhmm_fwdbwd_f32(const float* log_pi, const float* log_A, const float* em, const int64_t* lengths,
                     int64_t B, int64_t T, int64_t K, float* gamma, float* logZ, void* workspace,
                     size_t ws_bytes, void* stream);

/* ------------------------------------- causal filter, pairwise posteriors ----
 * Same inputs as Viterbi, 1 <= K <= 32 (larger K -> VQHMM_EUNSUPPORTED); hmm_pair.hip.
 *
 * vqhmm_filter_f32: filt (B,T,K) fp32 with filt[b,t,j] = p(z_t = j | x_{1:t}) (each row t < length
 * sums to 1; rows t >= length are 0) and loglik (B) fp32 = log p(x_{1:length}) (NaN if length 0,
 * as logZ).  The chain runs on linear probabilities normalised at every step; the logs of the step
 * masses are summed in fp64.  A step whose mass leaves [2^-30, 2^30] is redone as a max-shifted
 * log-sum-exp step; a sequence whose mass is truly 0 gets loglik = -inf (its filt from that step on
 * is unspecified) and leaves the other sequences untouched.  No workspace.
 * Accuracy target vs the fp64 oracle: |filt| abs 1e-5, loglik rel 1e-5.
 *
 * vqhmm_fwdbwd_xi_f32: gamma and logZ exactly as vqhmm_fwdbwd_f32 writes them (the same launch:
 * the same bits), and xi (B,T,K,K) fp32 with xi[b,t,i,j] = p(z_{t-1} = i, z_t = j | x_{1:length})
 * for 1 <= t < length, 0 at t = 0 and at t >= length (every element of xi is written).  Three
 * launches: forward-backward, the filter (into the workspace), then
 *   xi_t(i,j) = gamma_t(j) * filt_{t-1}(i) A_t(i,j) / sum_i' filt_{t-1}(i') A_t(i',j),
 * whose columns sum to gamma_t(j) by construction; a column whose denominator is 0 (structural
 * -inf in log_A) is 0, never NaN.  These are the gradients of logZ: d logZ / d log_A = xi,
 * d logZ / d em = gamma, d logZ / d log_pi = sum_b gamma[b,0].
 * Workspace: vqhmm_fwdbwd_xi_workspace_size(B, T, K) bytes (0 if K is unsupported).
 * Accuracy target vs the fp64 oracle: |xi| abs 2e-5.
 * Neither kernel reads outside [0, B*T*K*K) of log_A or [0, B*T*K) of em / gamma.
 * T = 0 (or B = 0) returns VQHMM_OK without a launch and writes nothing, loglik / logZ included. */
int vqhmm_filter_f32(const float* log_pi, const float* log_A, const float* em, const int64_t* lengths,
                     int64_t B, int64_t T, int64_t K, float* filt, float* loglik, void* stream);
size_t vqhmm_fwdbwd_xi_workspace_size(int64_t B, int64_t T, int64_t K);
int vqhmm_fwdbwd_xi_f32(const float* log_pi, const float* log_A, const float* em, const int64_t* lengths,
                        int64_t B, int64_t T, int64_t K, float* gamma, float* xi, float* logZ,
                        void* workspace, size_t ws_bytes, void* stream);

/* --------------------------------------------------- regime-path samplers ----
 * N state paths per sequence of the time-varying HMM over the Prior's tables (hmm_sample.hip):
 *   vqhmm_ffbs_sample_f32    z_{0:L-1} ~ p(z | x_{1:L}) by forward filtering, backward sampling, on
 *                            filt (B,T,K) as vqhmm_filter_f32 writes it;
 *   vqhmm_markov_sample_f32  z_0 ~ pi, z_t ~ A_t(z_{t-1}, .): simulation under the tables alone.
 * 1 <= K <= 32.  log_A (B,T,K,K) with log_A[:, t] the t-1 -> t transition, lengths (B) int64 clamped
 * to [0, T].  u (B,N,T) fp32 in [0,1): u[b,s,t] is the uniform that draws z_t of sample s.
 * paths (B,N,T) int32, every element written; -1 at t >= length.  No workspace.
 *
 * The draw rule (part of the contract; tests/sample_ref.py restates it).  Given fp32 weights
 * w_0 .. w_{K-1} >= 0: c_0 = w_0, c_i = c_{i-1} + w_i (a sequential fp32 sum in index order);
 * thr = u * c_{K-1} (one fp32 product); the draw is the smallest i with c_i > thr, or, if there is
 * none, the largest i with w_i > 0.  A state of weight 0 is therefore never drawn.  The draw FAILS
 * when c_{K-1} is 0 or not finite: that position gets -1, and so does every position the walk has
 * not yet reached in that sample.
 * The weights are shifted by the max, so a column or row whose entries are all tiny still samples:
 *   FFBS walks t = L-1 down to 0:  z_{L-1}: w_i = filt[b,L-1,i];  z_{t-1} given j = z_t:
 *     w_i = filt[b,t-1,i] * expf(log_A[b,t,i,j] - m), m = max_i log_A[b,t,i,j] (m = -inf fails);
 *   simulation walks t = 0 up to L-1:  z_0: w_i = expf(log_pi[i] - max log_pi);  z_t given
 *     i = z_{t-1}: w_j = expf(log_A[b,t,i,j] - max_j log_A[b,t,i,j]).
 * expf is the library function (within 1 ulp), not a fast intrinsic; the product and the sum are
 * separate roundings (no contraction).
 * The paths depend only on the inputs and u, never on the grid, the lane mapping or the kernel
 * variant; two calls give the same bits.  Every global access stays inside its own array (an
 * exact-size allocation is safe), offsets are 64-bit (B*N*T may pass 2^31).  NaN inputs may yield
 * any values in {-1, 0 .. K-1}.  filt / log_pi, log_A and u need only 4-byte alignment and give
 * the same paths as 16-byte aligned ones; paths must be 16-byte aligned.
 * Return codes, checked in this order on the host before any launch: a negative size ->
 * VQHMM_EINVAL; K outside [1, 32] -> VQHMM_EUNSUPPORTED; B*N*T == 0 -> VQHMM_OK without a launch;
 * a null pointer -> VQHMM_EINVAL.  (T > 2^28 or B >= 2^31: VQHMM_EUNSUPPORTED.) */
int vqhmm_ffbs_sample_f32(const float* filt, const float* log_A, const int64_t* lengths, const float* u,
                          int64_t B, int64_t T, int64_t K, int64_t N, int32_t* paths, void* stream);
int vqhmm_markov_sample_f32(const float* log_pi, const float* log_A, const int64_t* lengths, const float* u,
                            int64_t B, int64_t T, int64_t K, int64_t N, int32_t* paths, void* stream);

/* ----------------------------------------------- HMM on VQ code indices ----
 * The stationary discrete HMM of the pipeline's second half (pseudocode.txt:25-32: hmm.train_em on
 * the collected code indices, hmm.sample; math.md:23-62 with M_t = M; hmm_code.hip):
 * log_pi (S), log_A (S,S) with log_A[i,j] = log p(z_t = j | z_{t-1} = i), log_B (S,V) with
 * log_B[s,v] = log p(code = v | z = s), all fp32 natural logs; rows need not be normalised and
 * -inf is a structural zero.  1 <= S <= 32, 1 <= V <= 65536 (else VQHMM_EUNSUPPORTED, and the
 * workspace query returns 0).  codes (B,T) int32 as vqhmm_vq_argmin_f32 writes them, lengths (B)
 * int64 clamped to [0, T]; codes at t >= length are never interpreted.
 *
 * vqhmm_code_estep_f32: the Baum-Welch E-step in one call.  Every element of
 *   pi_cnt (S)      = sum_b gamma_{b,0}(s)
 *   trans_cnt (S,S) = sum_b sum_{1 <= t < L_b} xi_{b,t}(i,j)
 *   emit_cnt (S,V)  = sum_b sum_{t < L_b, codes[b,t] = v} gamma_{b,t}(s)
 * is written, in fp64 (the caller never clears them).  loglik (B) fp32 = log p(codes_{b,0:L_b})
 * (NaN for length 0) and gamma (B,T,S) fp32 (rows at t >= L are 0) are nullable; with gamma NULL
 * nothing of size B*T*S is written as output.  Neither per-step tables nor xi are materialised: the
 * chain runs on linear probabilities normalised at every step with the transition matrix in
 * registers and exp(log_B)^T in LDS (read through L2 when it does not fit), the step masses' logs
 * are summed in fp64, and a step whose mass leaves [2^-30, 2^30] is redone max-shifted in natural
 * log.  An impossible sequence (mass truly 0) gets loglik = -inf and a sequence with a code outside
 * [0, V) inside its length gets loglik = NaN; both contribute exactly 0 to every count, have zero
 * gamma rows and leave the other sequences untouched (log_B is never read out of range).
 * Deterministic: sequences are assigned to waves statically, each wave sums into a private slab and
 * the slabs are added in a fixed order in fp64; no float atomics.  Graph-capturable, no host sync.
 * B*T == 0 returns VQHMM_OK with the counts zeroed (and loglik = NaN for B > 0).
 * Workspace: vqhmm_code_estep_workspace_size(B, T, S, V) bytes (the scaled forward vectors,
 * 4*S bytes per position, the emission table and the slabs).
 * Accuracy target vs the fp64 oracle, per position: |gamma| abs 1e-5, |xi| abs 2e-5 (the counts
 * are their sums), loglik rel 1e-5 of max(1, |loglik|).
 * Reads stay inside [0, B*T) of codes and inside the parameter arrays.
 *
 * vqhmm_code_estep_batched_f32: the same E-step for a stack of M models (EM restarts, members of
 * different state counts padded with -inf, the components of a mixture) on one shared (codes,
 * lengths): log_pi (M,S), log_A (M,S,S), log_B (M,S,V) in, pi_cnt (M,S), trans_cnt (M,S,S),
 * emit_cnt (M,S,V) fp64, loglik (M,B) and gamma (M,B,T,S) (both nullable) out, all contiguous, the
 * member slices only 4-byte aligned.  The member is a grid dimension of the same kernel: the call
 * is three launches whatever M is, and member m's outputs are bit-identical to vqhmm_code_estep_f32
 * on member m's slices (which is the M = 1, weights = NULL case of it).  weights (M,B) fp32,
 * nullable (= all 1): member m's counts are sum_b weights[m,b] * (sequence b's counts under member
 * m), the product taken in fp64 as one fma where the contribution is added, so all-ones weights
 * give the bits of weights = NULL.  Weights may be negative or 0 and must be finite (a non-finite
 * weight leaves that member's counts unspecified, the other members' untouched); loglik and gamma
 * do not depend on them.  A sequence that is impossible or has a bad code under member m
 * contributes nothing to member m and normally to the others.  1 <= M <= 65535, else
 * VQHMM_EUNSUPPORTED (and the workspace query returns 0).  B*T == 0: as above, per member.
 * Workspace: vqhmm_code_estep_batched_workspace_size(B, T, S, V, M) bytes = M single-model
 * workspaces (each rounded up to 256 bytes).  Deterministic, graph-capturable, no host sync.
 *
 * vqhmm_code_sample_f32: ancestral sampling of N sequences of length T by inverse CDF from
 * caller-supplied uniforms (N,T,2) fp32 in [0,1): uniforms[n,t,0] draws z_t (from pi at t = 0, from
 * row z_{t-1} of A afterwards), uniforms[n,t,1] draws the code from row z_t of B.  The rule is part
 * of the contract: p_k = exp(log p_k) in fp32, cdf_k = the fp32 running sum in index order divided
 * by its own total, the draw is the first k with u < cdf_k, or the last k with p_k > 0 if there is
 * none; a zero-probability category is never drawn.  states (N,T), codes (N,T) int32.  No workspace.
 *
 * vqhmm_code_viterbi_f32 and vqhmm_code_filter_f32 (hmm_code_decode.hip): the MAP state path and the
 * causal filter of a code sequence, read from the 4-byte codes alone: no (B,T,S,S) / (B,T,S) table
 * is ever built, the transition matrix stays in registers for the whole sequence and the emission
 * table in LDS (read through L2 when S*V*4 > 64 KB).  Parameters, codes, lengths and the S, V limits
 * as above.
 *
 * vqhmm_code_viterbi_f32: path (B,T) int32, score (B) fp32.
 *   d_0[j] = log_pi[j] + log_B[j,c_0],  d_t[j] = (max_i (d_{t-1}[i] + log_A[i,j])) + log_B[j,c_t]
 * in fp32 in exactly this order, i ascending with a strict > (ties keep the lowest i); the last state
 * is the first argmax of d_{L-1}, score = d_{L-1}[last]; path[t >= L] = -1 and every element of path
 * is written.  L = 0: path all -1, score = -inf.  A code outside [0, V) inside the length: path all
 * -1, score = NaN, the other sequences untouched.  An impossible sequence gets what the rule gives:
 * score = -inf and the path of the tie rule.  For every sequence with valid codes the result is
 * bit-identical to vqhmm_viterbi_f32 on log_A[b,t] = log_A, em[b,t,j] = log_B[j, codes[b,t]].
 * Workspace: vqhmm_code_viterbi_workspace_size(B, T, S, V) bytes: one backpointer byte per step and
 * state (B * 4*ceil(T/4) * SP, SP = S rounded up to a power of two) and the (V,S) log_B^T table.
 *
 * vqhmm_code_filter_f32: filt (B,T,S) fp32 with filt[b,t,j] = p(z_t = j | codes_{b,0:t}) (rows
 * t < L sum to 1, rows t >= L are 0, every element written), last (B,S) = filt[b, L_b - 1] and
 * loglik (B) = log p(codes_{b,0:L_b} | prev); each of the three is nullable, and with filt NULL nothing
 * of size B*T*S is written (the streaming / scoring form).  prev (B,S), nullable, is the filtered
 * distribution at the position just before this chunk (non-negative, need not be normalised): the
 * distribution before the emission at t = 0 is exp(log_pi) with prev NULL and prev[b] . exp(log_A)
 * otherwise (log_pi is then not read and may be NULL), so feeding a call's last as the next call's prev
 * filters a feed chunk by chunk; last may alias prev.  L_b = 0: last[b] = prev[b] (zeros without
 * prev), loglik = NaN.  An impossible sequence (mass truly 0, or sum(prev[b]) = 0) gets loglik = -inf,
 * a code outside [0, V) inside the length loglik = NaN; in both cases the rows of filt from the
 * failing position on, and last, are 0, and the other sequences are untouched.  Numerics are the
 * E-step's forward (normalised every step, step masses' logs summed in fp64, max-shifted natural-log
 * step when a mass leaves [2^-30, 2^30]).  Workspace: vqhmm_code_filter_workspace_size(B, T, S, V)
 * bytes (the emission table).  Accuracy target vs the fp64 oracle: |filt|, |last| abs 1e-5, loglik
 * rel 1e-5 of max(1, |loglik|).
 *
 * Both: deterministic, graph-capturable, no host sync, 64-bit offsets, every global access inside
 * its own array (exact-size allocations and pointers misaligned by 4 bytes are safe).  Return
 * codes, checked in this order on the host before any launch: a negative size -> VQHMM_EINVAL; S or
 * V out of range -> VQHMM_EUNSUPPORTED; B > 0, T = 0 -> as if every length were 0 (the size-B outputs
 * are written); B = 0 -> VQHMM_OK; a null required pointer or a workspace that is too small ->
 * VQHMM_EINVAL. */
size_t vqhmm_code_viterbi_workspace_size(int64_t B, int64_t T, int64_t S, int64_t V);
int vqhmm_code_viterbi_f32(const float* log_pi, const float* log_A, const float* log_B,
                           const int32_t* codes, const int64_t* lengths,
                           int64_t B, int64_t T, int64_t S, int64_t V,
                           int32_t* path, float* score,
                           void* workspace, size_t ws_bytes, void* stream);
size_t vqhmm_code_filter_workspace_size(int64_t B, int64_t T, int64_t S, int64_t V);
int vqhmm_code_filter_f32(const float* log_pi, const float* log_A, const float* log_B,
                          const int32_t* codes, const int64_t* lengths, const float* prev,
                          int64_t B, int64_t T, int64_t S, int64_t V,
                          float* filt, float* last, float* loglik,
                          void* workspace, size_t ws_bytes, void* stream);
size_t vqhmm_code_estep_workspace_size(int64_t B, int64_t T, int64_t S, int64_t V);
int vqhmm_code_estep_f32(const float* log_pi, const float* log_A, const float* log_B,
                         const int32_t* codes, const int64_t* lengths,
                         int64_t B, int64_t T, int64_t S, int64_t V,
                         double* pi_cnt, double* trans_cnt, double* emit_cnt,
                         float* loglik, float* gamma,
                         void* workspace, size_t ws_bytes, void* stream);
size_t vqhmm_code_estep_batched_workspace_size(int64_t B, int64_t T, int64_t S, int64_t V, int64_t M);
int vqhmm_code_estep_batched_f32(const float* log_pi, const float* log_A, const float* log_B,
                                 const int32_t* codes, const int64_t* lengths, const float* weights,
                                 int64_t B, int64_t T, int64_t S, int64_t V, int64_t M,
                                 double* pi_cnt, double* trans_cnt, double* emit_cnt,
                                 float* loglik, float* gamma,
                                 void* workspace, size_t ws_bytes, void* stream);
int vqhmm_code_sample_f32(const float* log_pi, const float* log_A, const float* log_B,
                          const float* uniforms, int64_t N, int64_t T, int64_t S, int64_t V,
                          int32_t* states, int32_t* codes, void* stream);

/* ------------------------------------- Gaussian HMM on continuous data ----
 * The stationary HMM with diagonal-Gaussian emissions (hmm_gauss.hip): log_pi (S), log_A (S,S) with
 * log_A[i,j] = log p(z_t = j | z_{t-1} = i), mean (S,D), log_var (S,D), all fp32; rows of log_pi and
 * log_A need not be normalised and -inf there is a structural zero.  1 <= S <= 32, 1 <= D <= 64 (else
 * VQHMM_EUNSUPPORTED, and the workspace query returns 0).  x (B,T,D) fp32 row-major, lengths (B) int64
 * clamped to [0, T]; x at t >= length is never interpreted.
 *
 * vqhmm_gauss_emission_f32: em (B,T,S) fp32,
 *   em[b,t,s] = -1/2 sum_d ((x_d - mean_sd)^2 exp(-log_var_sd) + log_var_sd) - (D/2) ln 2 pi
 * computed as fma(-1/2, q, c_s): q the fp32 running sum over d in index order of fma((x_d - mean_sd)^2,
 * expf(-log_var_sd), q), c_s = -1/2 sum_d log_var_sd - (D/2) ln 2 pi summed in fp64 and rounded once.
 * Rows at t >= length are -inf; every element is written.  Accuracy target vs fp64 on the same fp32
 * inputs: (D + 16) 2^-23 (sum_d (z^2/2 + |log_var|/2) + (D/2) ln 2 pi).  No workspace.
 *
 * vqhmm_gauss_estep_f32: the Baum-Welch E-step in one call (two launches).  Every element of
 *   pi_cnt (S)      = sum_b w_b gamma_{b,0}(s)
 *   trans_cnt (S,S) = sum_b w_b sum_{1 <= t < L_b} xi_{b,t}(i,j)
 *   occ (S)         = sum_b w_b sum_{t < L_b} gamma_{b,t}(s)
 *   m1 (S,D)        = sum_b w_b sum_{t < L_b} gamma_{b,t}(s) (x_{b,t,d} - shift_d)
 *   m2 (S,D)        = sum_b w_b sum_{t < L_b} gamma_{b,t}(s) (x_{b,t,d} - shift_d)^2
 * is written, in fp64 (the caller never clears them).  shift (D) fp32 is nullable (= 0): moments about
 * a point near the data keep the M-step's variance from being a difference of two huge numbers.
 * weights (B) fp32 is nullable (w_b = 1): the product is one fp64 fma where the contribution is added
 * in fp64, so all-ones weights give the bits of weights = NULL; weights may be negative or 0 and must
 * be finite.  loglik (B) fp32 = log p(x_{b,0:L_b}) and gamma (B,T,S) fp32 (rows at t >= L are 0) are
 * nullable and do not depend on the weights; with gamma NULL nothing of size B*T*S is written as
 * output.  The emissions the chain uses are, bit for bit, what vqhmm_gauss_emission_f32 writes; they
 * are recomputed on chip from x in both passes (each step uses exp(em_t - max_s em_t), the maxima go
 * into the fp64 log-likelihood sum) and neither they nor xi reach memory.  The chain is
 * vqhmm_code_estep_f32's: linear probabilities normalised at every step, the transition matrix in
 * registers, a step whose mass leaves [2^-30, 2^30] redone max-shifted in natural log.  Length 0:
 * loglik = NaN.  An impossible sequence (mass truly 0): loglik = -inf.  A non-finite x or emission
 * inside the length: loglik = NaN.  All three contribute exactly 0 to every count, have zero gamma
 * rows and leave the other sequences untouched.  Deterministic (static assignment of sequences to
 * waves, private slabs, a fixed-order fp64 reduction launch, no float atomics), graph-capturable, no
 * host sync, 64-bit offsets, every global access inside its own array (exact-size allocations and
 * pointers misaligned by 4 bytes are safe).  Workspace: vqhmm_gauss_estep_workspace_size(B, T, S, D)
 * bytes (the scaled forward vectors, 4*S bytes per position, and the partial sums).
 * Accuracy target vs the fp64 oracle fed the same emissions, per position: |gamma| abs 1e-5, |xi| abs
 * 2e-5, loglik rel 1e-5 of max(1, |loglik|); m1 and m2 2e-5 of sum |x - shift| and sum (x - shift)^2.
 *
 * vqhmm_gauss_estep_batched_f32: the same E-step for a stack of M models (EM restarts, members of
 * different state counts padded with -inf, the components of a mixture) on one shared (x, lengths,
 * shift): log_pi (M,S), log_A (M,S,S), mean (M,S,D), log_var (M,S,D) in, pi_cnt (M,S), trans_cnt
 * (M,S,S), occ (M,S), m1 (M,S,D), m2 (M,S,D) fp64, loglik (M,B) and gamma (M,B,T,S) (both nullable)
 * out, all contiguous, the member slices only 4-byte aligned (the addressing guarantee above holds per
 * member).  The member is a grid dimension of the same two kernels: the call is two launches whatever
 * M is, each member runs the single model's schedule (which depends on B, T, S, D only), and member
 * m's outputs are bit-identical to vqhmm_gauss_estep_f32 on member m's slices (which is the M = 1 case
 * of it).  weights (M,B) fp32, nullable (= all 1): member m's counts are sum_b weights[m,b] *
 * (sequence b's counts under member m), the product taken in fp64 as one fma where the contribution is
 * added, so all-ones weights give the bits of weights = NULL.  Weights may be negative or 0 and must
 * be finite (a non-finite weight leaves that member's counts unspecified, the other members'
 * untouched); loglik and gamma do not depend on them.  The failure rules are per member: a sequence
 * of length 0, or that is impossible or meets a non-finite x or emission under member m, contributes
 * exactly 0 to member m, has zero gamma rows there and contributes normally to the others; under a
 * member whose own parameters are degenerate (a NaN log_var) every loglik is NaN and every count 0,
 * and its neighbours are bit-identical to the call without it.  1 <= M <= 65535, else
 * VQHMM_EUNSUPPORTED (and the workspace query returns 0); M < 0 -> VQHMM_EINVAL.  B*T == 0: as above,
 * per member.  Workspace: vqhmm_gauss_estep_batched_workspace_size(B, T, S, D, M) bytes = M
 * single-model workspaces (each rounded up to 256 bytes).  Each member stages x again.  Deterministic,
 * no float atomics, graph-capturable, no host sync, 64-bit offsets.
 *
 * vqhmm_gauss_sample_f32: ancestral sampling of N sequences of length T.  uniforms (N,T) fp32 in
 * [0,1) draw z_t by vqhmm_code_sample_f32's inverse-CDF rule (from pi at t = 0, from row z_{t-1} of A
 * afterwards); x[n,t,d] = fmaf(sd, normals[n,t,d], mean[z_t,d]) with sd = exp(log_var[z_t,d] / 2)
 * taken in fp64 and rounded once, normals (N,T,D) fp32 caller-supplied.  states (N,T) int32, x (N,T,D)
 * fp32.  Bit-reproducible given the draws.  No workspace.
 *
 * Return codes, checked in this order on the host before any launch: a negative size ->
 * VQHMM_EINVAL; S or D out of range -> VQHMM_EUNSUPPORTED (as are T > 2^28, B >= 2^31 and B*T > 2^40, for
 * which the workspace query returns 0 too); B*T == 0 (N*T == 0) -> VQHMM_OK without a
 * launch, the E-step's five counts zeroed (they must not be NULL: VQHMM_EINVAL) and loglik = NaN for
 * B > 0; a null required pointer or a workspace that is too small -> VQHMM_EINVAL. */
int vqhmm_gauss_emission_f32(const float* mean, const float* log_var,
                             const float* x, const int64_t* lengths,
                             int64_t B, int64_t T, int64_t S, int64_t D,
                             float* em, void* stream);
size_t vqhmm_gauss_estep_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D);
int vqhmm_gauss_estep_f32(const float* log_pi, const float* log_A,
                          const float* mean, const float* log_var,
                          const float* x, const int64_t* lengths,
                          const float* shift, const float* weights,
                          int64_t B, int64_t T, int64_t S, int64_t D,
                          double* pi_cnt, double* trans_cnt, double* occ, double* m1, double* m2,
                          float* loglik, float* gamma,
                          void* workspace, size_t ws_bytes, void* stream);
size_t vqhmm_gauss_estep_batched_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D, int64_t M);
int vqhmm_gauss_estep_batched_f32(const float* log_pi, const float* log_A,
                                  const float* mean, const float* log_var,
                                  const float* x, const int64_t* lengths,
                                  const float* shift, const float* weights,
                                  int64_t B, int64_t T, int64_t S, int64_t D, int64_t M,
                                  double* pi_cnt, double* trans_cnt, double* occ, double* m1, double* m2,
                                  float* loglik, float* gamma,
                                  void* workspace, size_t ws_bytes, void* stream);
int vqhmm_gauss_sample_f32(const float* log_pi, const float* log_A,
                           const float* mean, const float* log_var,
                           const float* uniforms, const float* normals,
                           int64_t N, int64_t T, int64_t S, int64_t D,
                           int32_t* states, float* x, void* stream);

/* ------------------------- Gaussian HMM with full covariances (hmm_gauss_full.hip) ----
 * The model of the block above with a full covariance per state: log_pi (S), log_A (S,S), mean (S,D)
 * as there, and prec_chol (S,D,D) fp32 row-major, W_s = L_s^-1 with Sigma_s = L_s L_s^T: lower-
 * triangular with a positive diagonal.  The strict upper triangle is never read.  1 <= S <= 32,
 * 1 <= D <= 32 and S*D*D <= 8192 (else VQHMM_EUNSUPPORTED, and the workspace queries return 0).  x,
 * lengths, shift and weights are the diagonal block's.
 *
 * vqhmm_gauss_full_emission_f32: em (B,T,S) fp32,
 *   em[b,t,s] = -1/2 |W_s (x - mean_s)|^2 + sum_i log W_s[i,i] - (D/2) ln 2 pi
 * computed as fma(-1/2, q, c_s): with z_j = x_j - mean_sj, r_i = the fp32 fma chain over j = 0..i in
 * index order of fma(W_s[i,j], z_j, r_i), q = the fma chain over i in index order of fma(r_i, r_i, q);
 * c_s = sum_i log W_s[i,i] - (D/2) ln 2 pi summed in fp64 and rounded once (a non-positive diagonal
 * makes c_s, and the state's emissions, NaN).  Rows at t >= length are -inf; every element is written.
 * Accuracy target vs fp64 on the same fp32 inputs: (3 D + 16) 2^-23 A with A = 1/2 sum_i (sum_{j<=i}
 * |W_ij| |z_j|)^2 + |sum_i log W_ii| + (D/2) ln 2 pi.  No workspace.
 *
 * vqhmm_gauss_full_estep_f32: vqhmm_gauss_estep_f32 with these emissions.  pi_cnt, trans_cnt, occ and
 * m1 are that entry's; the second moments are full,
 *   m2 (S,D,D) = sum_b w_b sum_{t < L_b} gamma_{b,t}(s) (x_{b,t,i} - shift_i) (x_{b,t,j} - shift_j):
 * the triangle j <= i is computed and written to [s,i,j] and [s,j,i], so m2 is symmetric bit for bit.
 * Every element of the five counts is written.  Everything else the diagonal entry states holds here
 * word for word: shift, weights (all ones = the bits of NULL), nullable loglik and gamma that do not
 * depend on the weights or on the rest of the batch, emissions that are bit for bit what
 * vqhmm_gauss_full_emission_f32 writes and never reach memory, the chain and its rare path, length 0 /
 * impossible / non-finite sequences (loglik NaN / -inf / NaN, zero contribution, zero gamma rows),
 * determinism, graph capture, 64-bit offsets, in-bounds access of exact-size and 4-byte-misaligned
 * buffers, and the accuracy targets, with m2[s,i,j] within 2e-5 of sum |x_i - shift_i| |x_j - shift_j|.
 * Workspace: vqhmm_gauss_full_estep_workspace_size(B, T, S, D) bytes.
 *
 * vqhmm_gauss_full_estep_batched_f32: vqhmm_gauss_estep_batched_f32 with these emissions, word for
 * word: prec_chol (M,S,D,D) in, m2 (M,S,D,D) out, the other arrays as there; two launches whatever M
 * is; member m bit-identical to vqhmm_gauss_full_estep_f32 on its slices (the M = 1 case); weights
 * (M,B); per-member failure rules (a member with a non-positive prec_chol diagonal has every loglik
 * NaN and every count 0, its neighbours untouched); 1 <= M <= 65535.  Workspace:
 * vqhmm_gauss_full_estep_batched_workspace_size(B, T, S, D, M) bytes = M single-model workspaces (each
 * rounded up to 256 bytes).
 *
 * vqhmm_gauss_moments_f32: occ (S), m1 (S,D) and m2 (S,D,D) as above, under a caller-supplied gamma
 * (B,T,S) fp32 (an encoder's posterior, a filter's output) in place of the chain's: the per-regime
 * weighted sums behind a pooled regime mean and covariance.  gamma at t >= length is never read.  A
 * sequence with a non-finite x or gamma inside its length contributes exactly 0.  Three launches (the
 * flags of such sequences, one wave per sequence and 64-step chunk, the E-step's fixed-order
 * reduction); deterministic, no atomics, graph-capturable, same addressing guarantees.  Workspace:
 * vqhmm_gauss_moments_workspace_size(B, T, S, D) bytes.
 *
 * Return codes: the diagonal block's, in its order.  B*T == 0 -> VQHMM_OK without a launch, the counts
 * (E-step: five, moments: three; they must not be NULL: VQHMM_EINVAL) zeroed and loglik = NaN for
 * B > 0. */
int vqhmm_gauss_full_emission_f32(const float* mean, const float* prec_chol,
                                  const float* x, const int64_t* lengths,
                                  int64_t B, int64_t T, int64_t S, int64_t D,
                                  float* em, void* stream);
size_t vqhmm_gauss_full_estep_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D);
int vqhmm_gauss_full_estep_f32(const float* log_pi, const float* log_A,
                               const float* mean, const float* prec_chol,
                               const float* x, const int64_t* lengths,
                               const float* shift, const float* weights,
                               int64_t B, int64_t T, int64_t S, int64_t D,
                               double* pi_cnt, double* trans_cnt, double* occ, double* m1, double* m2,
                               float* loglik, float* gamma,
                               void* workspace, size_t ws_bytes, void* stream);
size_t vqhmm_gauss_full_estep_batched_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D, int64_t M);
int vqhmm_gauss_full_estep_batched_f32(const float* log_pi, const float* log_A,
                                       const float* mean, const float* prec_chol,
                                       const float* x, const int64_t* lengths,
                                       const float* shift, const float* weights,
                                       int64_t B, int64_t T, int64_t S, int64_t D, int64_t M,
                                       double* pi_cnt, double* trans_cnt, double* occ, double* m1, double* m2,
                                       float* loglik, float* gamma,
                                       void* workspace, size_t ws_bytes, void* stream);
size_t vqhmm_gauss_moments_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D);
int vqhmm_gauss_moments_f32(const float* x, const float* gamma, const int64_t* lengths,
                            const float* shift, const float* weights,
                            int64_t B, int64_t T, int64_t S, int64_t D,
                            double* occ, double* m1, double* m2,
                            void* workspace, size_t ws_bytes, void* stream);

/* ------------------- Gaussian HMM: Viterbi decode and streaming causal filter on x ----
 * The MAP state path and the causal filter of both Gaussian models (hmm_gauss_decode_dev.h, instantiated
 * next to the emission code of hmm_gauss.hip and hmm_gauss_full.hip), read from x alone: a wave stages 64
 * rows of x in LDS, computes their emissions on chip with the function the emission entry uses and runs
 * the chain on them, the transition matrix in registers.  No (B,T,S) emission table, no expanded log_A
 * and no xi reaches memory.  Parameters, x, lengths and the limits are the two blocks' above: diagonal
 * 1 <= S <= 32, 1 <= D <= 64 with log_var (S,D); full 1 <= S <= 32, 1 <= D <= 32, S*D*D <= 8192 with
 * prec_chol (S,D,D); T <= 2^28, B < 2^31, B*T <= 2^40 (else VQHMM_EUNSUPPORTED, and the workspace query
 * returns 0).
 *
 * vqhmm_gauss_viterbi_f32 / vqhmm_gauss_full_viterbi_f32: path (B,T) int32, score (B) fp32.
 *   d_0[j] = log_pi[j] + em[0,j],  d_t[j] = (max_i (d_{t-1}[i] + log_A[i,j])) + em[t,j]
 * in fp32 in exactly this order on the raw log emissions (no max shift), i ascending with a strict >
 * (ties keep the lowest i); the last state is the first argmax of d_{L-1}, score = d_{L-1}[last];
 * path[t >= L] = -1 and every element of path is written.  L = 0: path all -1, score = -inf.  A
 * non-finite x or emission inside the length: path all -1, score = NaN, the other sequences untouched.
 * An impossible sequence gets what the rule gives: score = -inf and the path of the tie rule.  For
 * every sequence with finite data the result is bit-identical to vqhmm_viterbi_f32 on log_A[b,t] = log_A
 * and em as vqhmm_gauss_emission_f32 (vqhmm_gauss_full_emission_f32) writes it.  Workspace:
 * vqhmm_gauss_viterbi_workspace_size / vqhmm_gauss_full_viterbi_workspace_size (B, T, S, D) bytes: one
 * backpointer byte per step and state, B * 4*ceil(T/4) * SP with SP = S rounded up to a power of two,
 * rounded up to 256; the only per-position workspace.
 *
 * vqhmm_gauss_filter_f32 / vqhmm_gauss_full_filter_f32: filt (B,T,S) fp32 with filt[b,t,j] = p(z_t = j |
 * x_{b,0:t}) (rows t < L sum to 1, rows t >= L are 0, every element written), last (B,S) = filt[b, L_b - 1]
 * and loglik (B) = log p(x_{b,0:L_b} | prev); each of the three is nullable, and with filt NULL nothing of
 * size B*T*S is written (the streaming / scoring form).  No workspace.  prev (B,S), nullable, is the
 * filtered distribution at the position just before this chunk (non-negative, need not be normalised):
 * the distribution before the emission at t = 0 is exp(log_pi) with prev NULL and prev[b] . exp(log_A)
 * otherwise (log_pi is then not read and may be NULL), so feeding a call's last as the next call's prev
 * filters a feed chunk by chunk; last may alias prev.  L_b = 0: last[b] = prev[b] (zeros without prev),
 * loglik = NaN.  An impossible sequence (mass truly 0, or sum(prev[b]) equal to 0 or not finite) gets
 * loglik = -inf; the first position inside the length whose row of x, or whose emission, is not finite
 * gives loglik = NaN, and the steps before that position still run; in both cases the rows of filt from
 * the failing position on, and last, are 0, and the other sequences are untouched.  Numerics are the
 * E-step's forward: each step uses exp(em_t - max_s em_t), the maxima go into the fp64 log-likelihood
 * sum, linear probabilities are normalised at every step, four step masses go through one log2 into
 * fp64, a step whose mass leaves [2^-30, 2^30] is redone max-shifted in natural log.  Accuracy target vs
 * the fp64 oracle fed the same emissions: |filt|, |last| abs 1e-5, loglik rel 1e-5 of max(1, |loglik|).
 *
 * All four: deterministic, graph-capturable, no host sync, 64-bit offsets, every global access inside
 * its own array (x only at rows t < L; exact-size allocations and pointers misaligned by 4 bytes are
 * safe).  Return codes, checked in this order on the host before any launch: a negative size ->
 * VQHMM_EINVAL; S, D or the batch out of range -> VQHMM_EUNSUPPORTED; B = 0 -> VQHMM_OK; B > 0, T = 0 ->
 * as if every length were 0 (the size-B outputs are written); a null required pointer or a workspace
 * that is too small -> VQHMM_EINVAL. */
size_t vqhmm_gauss_viterbi_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D);
int vqhmm_gauss_viterbi_f32(const float* log_pi, const float* log_A,
                            const float* mean, const float* log_var,
                            const float* x, const int64_t* lengths,
                            int64_t B, int64_t T, int64_t S, int64_t D,
                            int32_t* path, float* score,
                            void* workspace, size_t ws_bytes, void* stream);
int vqhmm_gauss_filter_f32(const float* log_pi, const float* log_A,
                           const float* mean, const float* log_var,
                           const float* x, const int64_t* lengths, const float* prev,
                           int64_t B, int64_t T, int64_t S, int64_t D,
                           float* filt, float* last, float* loglik, void* stream);
size_t vqhmm_gauss_full_viterbi_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D);
int vqhmm_gauss_full_viterbi_f32(const float* log_pi, const float* log_A,
                                 const float* mean, const float* prec_chol,
                                 const float* x, const int64_t* lengths,
                                 int64_t B, int64_t T, int64_t S, int64_t D,
                                 int32_t* path, float* score,
                                 void* workspace, size_t ws_bytes, void* stream);
int vqhmm_gauss_full_filter_f32(const float* log_pi, const float* log_A,
                                const float* mean, const float* prec_chol,
                                const float* x, const int64_t* lengths, const float* prev,
                                int64_t B, int64_t T, int64_t S, int64_t D,
                                float* filt, float* last, float* loglik, void* stream);

/* ------------------- Gaussian HMM scenarios: Monte Carlo paths with on-chip RNG ----
 * vqhmm_gauss_scenario_f32 (hmm_gauss_scenario.hip): from a regime distribution per start to N simulated
 * paths of H steps per start, in one launch: the regime chain, the Gaussian returns and a portfolio's
 * wealth path, with every random number generated on chip.  start (B,S) fp32: non-negative weights of
 * the regime at simulated step 0 (need not be normalised).  log_A (S,S), mean (S,D) as above.  scale:
 * full = 0: (S,D) standard deviations; full = 1: (S,D,D) row-major lower Cholesky factors L (Sigma = L
 * L^T), of which only the lower triangle is read.  1 <= S <= 32; D <= 64 (full = 0); D <= 32 and S*D*D <=
 * 8192 (full = 1); H <= 2^28, B*N <= 2^36, B*N*H <= 2^48 (else VQHMM_EUNSUPPORTED).  port (S,D) fp32,
 * nullable: the holdings taken when a rebalance finds the path in that regime.  Path (b, n) is path
 * (b0 + b, n0 + n) of the seed's stream: a call on a sub-range of starts or paths returns the bits of the
 * full call's rows.
 *
 * Outputs, each nullable, at least one not: states (B,N,H) int32, x (B,N,H,D) fp32, wealth (B,N,H) fp32,
 * final_wealth (B,N) fp32, drawdown (B,N) fp32.  wealth, final_wealth and drawdown need port.  What is
 * written does not depend on which other outputs are asked for.
 *
 * Random numbers: Philox4x32-10 (Random123: multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 * 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32), counter = (n0 + n, b0 + b, t, j).  Block j = 0: its
 * word 0, w, gives the regime uniform u = (w >> 8) * 2^-24.  Block j = 1 + d / 4 (integer division) gives
 * the normals of dimensions 4 (j - 1) .. 4 (j - 1) + 3 by Box-Muller on the word pairs (0,1) and (2,3):
 * u1 = ((wa >> 8) + 1) * 2^-24, u2 = (wb >> 8) * 2^-24, r = sqrtf(-2 logf(u1)), eps = r cospif(2 u2) for
 * the even and r sinpif(2 u2) for the odd dimension.  u1 >= 2^-24, so the tails are cut at |eps| <= sqrt(48
 * ln 2) = 5.77 (mass 8e-9 per draw).
 *
 * Chain: z_0 is drawn from p_k = start[b,k], z_t from p_k = expf(log_A[z_{t-1}, k]), by
 * vqhmm_code_sample_f32's rule: the first k with p_k > 0 and u < run_k / total (run the fp32 running sum
 * in index order, total its last value), else the last k with p_k > 0; a zero weight is never drawn.  A
 * negative or non-finite entry of start[b], or a total (of start[b], or of the row entered) that is 0 or
 * not finite, fails the path from that step on: states = -1 and x = wealth = NaN from there, final_wealth
 * = drawdown = NaN; the other paths are untouched.
 *
 * Returns: full = 0: x[d] = fmaf(scale[z,d], eps_d, mean[z,d]); full = 1: x[i] = the fp32 fma chain acc =
 * mean[z,i], acc = fmaf(L[z,i,j], eps_j, acc) for j = 0..i in index order.
 *
 * Wealth, carried in fp64: w = 1, peak = 1, dd = 0, nothing held.  At t % rebalance == 0: w -= w * tx_cost *
 * sum_d |port[z_t,d] - held_d| (the sum in fp64 in index order), then held = port[z_t].  Every step: w *=
 * 1 + sum_d held_d x[t,d] (fp64, index order, on the fp32 x); wealth[b,n,t] = (float) w; peak = max(peak,
 * w); dd = max(dd, 1 - w / peak).  final_wealth = (float) w after the last step (the bits of wealth[b,n,
 * H-1]), drawdown = (float) dd.
 *
 * No workspace, no host sync, deterministic, graph-capturable, 64-bit offsets, every global access inside
 * its own array.  Return codes, checked in this order on the host before any launch: a negative size (B,
 * N, H, S, D, b0, n0) -> VQHMM_EINVAL; S, D or the sizes out of range -> VQHMM_EUNSUPPORTED; B*N*H == 0
 * -> VQHMM_OK without a launch; a null required pointer (start, log_A, mean, scale; port with a wealth
 * output; every output NULL), rebalance < 1, or b0 + B or n0 + N above 2^32 -> VQHMM_EINVAL. */
int vqhmm_gauss_scenario_f32(const float* start, const float* log_A, const float* mean,
                             const float* scale, int full, const float* port,
                             int64_t rebalance, float tx_cost, uint64_t seed,
                             int64_t b0, int64_t n0,
                             int64_t B, int64_t N, int64_t H, int64_t S, int64_t D,
                             int32_t* states, float* x, float* wealth,
                             float* final_wealth, float* drawdown, void* stream);

/* ------------------- Historical back-test: wealth and its statistics over windows x policies ----
 * vqhmm_backtest_f32 (hmm_backtest.hip): a regime-conditional portfolio run through B historical windows
 * under P policies, with rebalancing and transaction costs, in one launch.  returns (B,T,D) fp32; probs
 * (B,T,S) fp32, any per-step regime distribution (a filter's, a smoother's, an encoder's), not
 * renormalised; lengths (B) int64, nullable (= T; clamped to [0, T]); weights (P,S,D) fp32; rebalance (P)
 * int32 >= 1 (a value below 1 is read as 1); tx_cost (P) fp32 >= 0; lag >= 0; hard 0 / 1.  1 <= S <= 32,
 * 1 <= D <= 64, B, T, P >= 0; T <= 2^28, P <= 2^24, B*P < 2^31 (else VQHMM_EUNSUPPORTED).  Every
 * arithmetic step from the fp32 inputs is fp64; the order of sums and products is not specified.
 *
 * Per window b and policy p, with L the length, R = rebalance[p], c = tx_cost[p], W = weights[p]:
 *   V = 1, peak = 1, dd = 0, held = 0 (a D-vector), i = -1
 *   for t = 0 .. L-1:
 *     tau = 0
 *     if t >= lag and (t - lag) % R == 0:
 *       q = probs[b, t - lag]
 *       target = sum_s q[s] W[s,:]            (hard = 0)
 *              = W[argmax_s q[s], :]          (hard = 1; the lowest index among equal maxima)
 *       tau = sum_d |target_d - held_d|;  held = target
 *     g   = sum_d held_d returns[b,t,d]
 *     rho = (1 - c tau) (1 + g) - 1           (the step's net return)
 *     V   = V (1 + rho)
 *     if V > peak: peak = V, i = t
 *     if V < peak and 1 - V/peak > dd: dd = 1 - V/peak, i* = i, j* = t
 * Before step `lag` nothing is held and rho = 0 exactly; lag = 0 trades step t on a row that saw step t.
 * No clamp where c tau >= 1.  An equal later drawdown does not replace an earlier one.
 *
 * stats (B,P,12) fp64, columns: final (V after step L-1), n (= L), sum (of rho), sumsq (of rho^2), n_neg
 * (steps with rho < 0), sum_neg, sumsq_neg (over those steps), n_pos (steps with rho > 0), drawdown (dd >=
 * 0), turnover (sum of tau), t_peak (i*), t_trough (j*; both -1 when dd = 0).  L = 0: final 1, the rest 0
 * and -1, -1.  A non-finite value of returns[b, t, :] or probs[b, t, :] at any t < L makes all twelve
 * columns of window b NaN for every policy.  wealth (B,P,T) fp32, nullable: V after step t rounded once,
 * 0 at t >= L; wealth[b,p,L-1] has the bits of (float) final; NaN at t < L in a failed window.
 *
 * stats[b,p] and wealth[b,p] are functions of window b's inputs up to its length and of policy p's weights,
 * rebalance and tx_cost alone: a call on a slice of the windows or of the policies, a call with or without
 * wealth, and a call with another T beyond the lengths return the same bits.
 *
 * vqhmm_backtest_bwd_f32: grad_weights (P,S,D) fp64 = dLoss/dweights given grad_stats (B,P,12) fp64 =
 * dLoss/dstats, by recomputing the forward pass (nothing is saved).  The columns n, n_neg, n_pos, t_peak,
 * t_trough carry no gradient; returns and probs receive none.  With g_x the incoming gradient of column x,
 * the adjoint of step t's net return is
 *   a_t = g_sum + 2 rho_t g_sumsq + [rho_t < 0] (g_sum_neg + 2 rho_t g_sumsq_neg)
 *         + g_final V_L / (1 + rho_t) - g_drawdown [i* < t <= j*] (V_j* / V_i*) / (1 + rho_t)     (V_-1 = 1)
 * and with u_k = g_turnover - c (1 + g_k) a_k at rebalance date k, h_k the holdings taken there (0 before
 * the first date, sign(0) = 0), the adjoint of h_k is
 *   abar_k = sum_{t in k's holding period} a_t (1 - c tau_t) returns[b,t,:]
 *            + u_k sign(h_k - h_{k-1}) - u_{k+1} sign(h_{k+1} - h_k)
 * and grad_weights[p,s,:] = sum over windows and dates of q_k[s] abar_k (hard = 1: abar_k is added to row
 * argmax q_k).  The sum over windows is deterministic: fp64 partials per tile of 8 windows in the workspace
 * (vqhmm_backtest_bwd_workspace_size bytes), added in tile order by a second launch; two identical calls
 * return identical bits, and a call on a slice of the policies returns the full call's rows.  A failed
 * window contributes NaN.  grad_weights is written, not accumulated into (B = 0: zeros).
 *
 * No host sync, graph-capturable, 64-bit offsets, every global access inside its own array.  Return codes,
 * checked in this order on the host before any launch: a negative size (B, T, S, D, P, lag) ->
 * VQHMM_EINVAL; S, D or the sizes out of range -> VQHMM_EUNSUPPORTED (the workspace query returns 0); B*P
 * == 0 -> VQHMM_OK without a launch (the backward entry with B = 0 < P zeroes grad_weights); a null
 * required pointer (stats / grad_weights, weights, rebalance, tx_cost; returns and probs when T > 0;
 * grad_stats and workspace when B > 0) -> VQHMM_EINVAL.  The values of rebalance and tx_cost are device
 * data and are not checked. */
int vqhmm_backtest_f32(const float* returns, const float* probs, const int64_t* lengths,
                       const float* weights, const int32_t* rebalance, const float* tx_cost,
                       int64_t lag, int hard,
                       int64_t B, int64_t T, int64_t S, int64_t D, int64_t P,
                       double* stats, float* wealth, void* stream);
size_t vqhmm_backtest_bwd_workspace_size(int64_t B, int64_t T, int64_t S, int64_t D, int64_t P);
int vqhmm_backtest_bwd_f32(const float* returns, const float* probs, const int64_t* lengths,
                           const float* weights, const int32_t* rebalance, const float* tx_cost,
                           int64_t lag, int hard,
                           int64_t B, int64_t T, int64_t S, int64_t D, int64_t P,
                           const double* grad_stats, double* grad_weights,
                           void* workspace, void* stream);

/* -------------------------------------------------- codebook learning ----
 * Per-code statistics of a batch under given assignments, the quantizer's backward from the same
 * pass, and the channels-first lookup (pseudocode.txt:8-32, the codebook's side; vq_codebook.hip).
 * z (B,Dv,T) channels-first fp32, idx (B,T) int32 as vqhmm_vq_argmin_f32 writes them, lengths (B)
 * int64 (nullable: every t counts), codebook (K,Dv) fp32.  1 <= K <= 65536, 1 <= Dv <= 512,
 * K*Dv <= 2^21 (else VQHMM_EUNSUPPORTED, and the workspace queries return 0).
 *
 * A position (b,t) counts when t < clamp(lengths[b], 0, T) and 0 <= idx[b,t] < K; idx at
 * t >= length is never read.  Its residual is r_d = fl32(z[b,d,t] - codebook[idx[b,t]][d]).
 *
 * vqhmm_vq_stats_f32: every element of
 *   count[k]  (K)    = the number of counted positions with idx = k
 *   rsum[k,d] (K,Dv) = sum of r_d over those positions
 *   *sse      (1, nullable) = sum of r_d^2 over all counted positions
 * is written, in fp64 (the caller never clears them).  The residual form serves every update rule
 * without the cancellation of sum z - count c: the codebook gradient of the MSE is -(2 g / n) rsum,
 * the per-code mean is c + rsum / count, the plain sum is rsum + count c.
 *
 * vqhmm_vq_quantize_bwd_f32: the same pass, writing
 *   dz[b,d,t]      = fl(g + fl(s * r_d))    g = g_zq[b,d,t] (0 with g_zq NULL), s = *dz_scale,
 *                                           r_d = 0 at positions that do not count
 *   dcodebook[k,d] = (float)(*dcb_scale * rsum[k,d])    (the product in fp64)
 * dz (B,Dv,T) and dcodebook (K,Dv) are each nullable; every element of the ones given is written; dz
 * may alias g_zq.  dz is two fp32 roundings, never contracted.  dz_scale and dcb_scale point to device
 * floats, so a caller whose scales are device scalars (autograd's incoming gradients) needs no host
 * sync.  With s = 2 beta g_commit / n and *dcb_scale = -2 g_cb / n this is the backward of
 * vqhmm_vq_quantize_f32's two losses over n = B Dv T elements plus the straight-through gradient.
 *
 * Accumulation: every addition into a bin is fp64, made in position order by the one lane that owns
 * the bin's channel in the one wave that owns the bin's code; tiles of 64 positions are assigned to
 * workgroups statically, each workgroup fills one slab and a second launch adds the workgroups'
 * slabs in a fixed order.  No float atomics: the same inputs give the same bits every run.
 * The slab lives in LDS when (K*Dv + K + 1)*8 bytes fit beside the 16.25 KB staging tile (K*(Dv+1) <= 17887: 256 x 64, 512 x 32)
 * and in the workgroup's partial in the workspace otherwise.  Graph-capturable, no host sync, 64-bit
 * offsets, z / g_zq / dz touched only at t < T, the codebook only at rows in [0, K).
 * Workspace: vqhmm_vq_stats_workspace_size / vqhmm_vq_quantize_bwd_workspace_size bytes (the
 * partials, at most 64 MB unless one partial is larger).
 *
 * vqhmm_vq_lookup_f32: out[b,d,t] = codebook[idx[b,t]][d] (B,Dv,T) fp32, 0 where idx is outside
 * [0, K) (vqhmm_code_viterbi_f32's and CodeHMM's -1 padding); every element written.  No workspace.
 *
 * Return codes, checked in this order on the host before any launch: a negative size ->
 * VQHMM_EINVAL; K, Dv or K*Dv out of range -> VQHMM_EUNSUPPORTED; B*T == 0 -> VQHMM_OK with the
 * given outputs zeroed and no kernel launch; a null required pointer (z, idx, codebook, count, rsum;
 * dz_scale, dcb_scale; out) -> VQHMM_EINVAL; a null or short workspace -> VQHMM_EWORKSPACE. */
size_t vqhmm_vq_stats_workspace_size(int64_t B, int64_t Dv, int64_t T, int64_t K);
int vqhmm_vq_stats_f32(const float* z, const int32_t* idx, const int64_t* lengths,
                       int64_t B, int64_t Dv, int64_t T, const float* codebook, int64_t K,
                       double* count, double* rsum, double* sse,
                       void* workspace, size_t ws_bytes, void* stream);
size_t vqhmm_vq_quantize_bwd_workspace_size(int64_t B, int64_t Dv, int64_t T, int64_t K);
int vqhmm_vq_quantize_bwd_f32(const float* z, const int32_t* idx, const int64_t* lengths,
                              int64_t B, int64_t Dv, int64_t T, const float* codebook, int64_t K,
                              const float* g_zq, const float* dz_scale, const float* dcb_scale,
                              float* dz, float* dcodebook,
                              void* workspace, size_t ws_bytes, void* stream);
int vqhmm_vq_lookup_f32(const float* codebook, int64_t K, int64_t Dv, const int32_t* idx,
                        int64_t B, int64_t T, float* out, void* stream);

/* ------------------------------------------------------- training step ----
 * compute_loss forward + backward of VAE_HMM (VQ_VAE_HMM_fixed.py:106-137,
 * autograd of :156) as one native executor over hand-written kernels.
 *
 * params: host array of VQHMM_NPARAMS device pointers in parameters() order
 *   (shapes: the reference's nn.Conv1d / nn.Linear / nn.Embedding weights).
 * x (B, D, T) CF; u (B, U, T) if u_layout == 0, (B, T, U) if u_layout == 1
 *   (Prior.forward's permute rule, :64-65); lengths (B) int64 on device.
 * Workspace: vqhmm_elbo_workspace_size(); the forward saves activations in it
 * and the backward must get the same workspace, dims, B and T.
 * loss: device fp32 scalar; loss_accum (nullable): device fp64 scalar += loss
 *   (train_model's epoch_loss, :158, without a per-step host sync).
 * need_grad = 0 computes only the loss; 2 = as 1, but the loss (and loss_accum) are left to the
 *   backward: vqhmm_elbo_bwd_adam_f32 or vqhmm_elbo_bwd_loss_f32 with its loss pointers finalizes
 *   them in its own last launch (one launch fewer per step).
 * norm: NULL, or a device int64[2] {valid_count, batch} replacing the batch's own
 *   loss normalisers mask.sum() (:120) and B (:131, :135).  Pass the GLOBAL batch's
 *   values when this batch is one shard of it: the shards' losses and gradients then
 *   SUM to the global batch's exactly (data parallel over ragged batches).  The
 *   backward must get the same norm as its forward.
 * Backward: grad (flat fp32, vqhmm_param_layout order) = grad_scale * dloss/dparams,
 *   grad_scale a device fp32 scalar (autograd's grad_output) or NULL for 1. */
int vqhmm_elbo_workspace_size(const vqhmm_dims_t* dims, int64_t B, int64_t T, size_t* bytes);
int vqhmm_elbo_fwd_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                       const float* u, int u_layout, const int64_t* lengths, const int64_t* norm, int64_t B, int64_t T,
                       float beta, int need_grad, void* workspace, size_t ws_bytes,
                       float* loss, double* loss_accum, void* stream);
int vqhmm_elbo_bwd_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                       const int64_t* norm, int64_t B, int64_t T, float beta, const float* grad_scale,
                       void* workspace, size_t ws_bytes, float* grad, void* stream);
/* vqhmm_elbo_bwd_f32 that also finalizes the loss of a forward run with need_grad = 2 into loss /
 * loss_accum (the data-parallel step form: forward + backward, then the gradient all-reduce and
 * vqhmm_adam_f32; VQ_VAE_HMM_fixed.py:137,156,158). */
int vqhmm_elbo_bwd_loss_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                            const int64_t* norm, int64_t B, int64_t T, float beta, const float* grad_scale,
                            void* workspace, size_t ws_bytes, float* grad, float* loss, double* loss_accum,
                            void* stream);
/* Backward + torch.optim.Adam step (the single-process train_model step,
 * VQ_VAE_HMM_fixed.py:155-157): vqhmm_elbo_bwd_f32 (grad_scale NULL) whose last launch
 * also applies vqhmm_adam_f32's update to every parameter element (same formula, same
 * device step counter and ticket), saving the separate update launch; grad still receives
 * the full gradient.  params[i] must be param + offset[i] of vqhmm_param_layout (the flat
 * buffer Adam updates in place).  adam_grad_scale multiplies the gradient inside Adam only.
 * loss / loss_accum: NULL, or (after a forward with need_grad = 2) where the forward's loss is
 * finalized, as vqhmm_elbo_fwd_f32 would have. */
int vqhmm_elbo_bwd_adam_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                            const int64_t* norm, int64_t B, int64_t T, float beta, void* workspace,
                            size_t ws_bytes, float* grad, float* param, float* exp_avg, float* exp_avg_sq,
                            double lr, double beta1, double beta2, double eps, int64_t* step,
                            float adam_grad_scale, float* loss, double* loss_accum, void* stream);
/* Device addresses (inside the workspace) of the last forward's loss and of its
 * pieces [recon, prior, entropy] (for tests).  Host-only, no GPU access. */
int vqhmm_elbo_pieces(const vqhmm_dims_t* dims, int64_t B, int64_t T, const void* workspace,
                      const float** loss, const float** pieces);

/* Byte offset, inside an elbo workspace of this (dims, B, T), of the step's 8-byte device
 * status word (VQHMM_STATUS_* bits).  The caller zeroes it once after allocating the
 * workspace; the step's kernels never clear it.  Host-only. */
int vqhmm_elbo_status_offset(const vqhmm_dims_t* dims, int64_t B, int64_t T, size_t* offset);

/* Device addresses (inside the workspace) of the step's PCL activation and gradient
 * buffers, in this order: x, h1, h2, logits, q, g1, g2, par (mu|logvar), dpar, dg2, dg1,
 * dq(decoder), dlogits, dh2, dh1, dq(prior).  Row r = b*(T+2)+1+t, stride ld4(channels).
 * Host-only, for accuracy diagnostics (tools/grad_accuracy.py). */
int vqhmm_elbo_debug_buffers(const vqhmm_dims_t* dims, int64_t B, int64_t T, const void* workspace,
                             const float** buffers16);

/* Phase timestamps (s_memrealtime ticks, 100 MHz) of the last launch of a kernel family built for
 * profiling (which = 0: the strip kernels, VQHMM_STRIP_PROF=1; 1: the conv2 kernels, VQHMM_CONV_PROF=1;
 * 2: the cooperative ELBO head, VQHMM_HEAD_PROF=1;
 * the switches are read once; results unchanged): 16 slots per workgroup for the first 256
 * workgroups.  Host-only, synchronous (tools/strip_prof.py). */
int vqhmm_debug_prof(int which, uint64_t* out, int64_t n);

/* Stage table of the training step (forward stages then backward stages, in
 * launch order).  stage_info: name, algorithmic FLOPs and bytes of ONE launch
 * (host-only); stage_f32 re-runs one stage on a workspace holding a completed
 * forward/backward (per-kernel timing, ablation). */
int vqhmm_elbo_num_stages(void);
int vqhmm_elbo_stage_info(const vqhmm_dims_t* dims, int64_t B, int64_t T, int stage, char* name,
                          size_t name_len, double* flops, double* bytes, int* mfma_bound);
/* Which kernel family the stage's launch runs for these dims and this (B, T): a short stable string
 * (host-only, read-only; the launchers take their decision from the same functions).
 *   convolutions      "conv2", "convbig", "convbig+tail", "conv_mm<BM,BN,KCH>" (the generic implicit GEMM and
 *                     its tile), "...+tail" (fused 1x1 tail), "...+tail_kernel" (the tail as a second launch,
 *                     N > 256), "fused_pair", "bwd_pair", "strip_fwd", "strip_bwd", "strip_bwdw";
 *                     dec_conv1's data gradient adds "+logits_bwd[+logits_dg]" for what rides in its epilogue,
 *                     and the stages that ride there report its family
 *   weight gradients  "wgrad2", "wgrad2_group", "strip_bwdw", "wgradbig", "wgrad_generic"
 *   the ELBO head     "pipe", "coop", "mfma", "scalar", "strip_fwd", or
 *                     "staged:<l1 kernel>;hid=<conv>;lgA=<conv>;dhid=<conv>;dW1=<wgrad>;dW2=<wgrad>"
 * "unsupported" where the stage's launch would return VQHMM_EUNSUPPORTED.  The string is truncated to
 * len - 1 characters. */
int vqhmm_elbo_stage_family(const vqhmm_dims_t* dims, int64_t B, int64_t T, int stage, char* family, size_t len);
int vqhmm_elbo_stage_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                         const float* u, int u_layout, const int64_t* lengths, const int64_t* norm,
                         int64_t B, int64_t T, float beta, void* workspace, size_t ws_bytes, float* grad, int stage,
                         void* stream);

/* torch.optim.Adam step (no weight decay / amsgrad; train_model uses the
 * defaults, :146) over n contiguous fp32 elements.  `step` is a DEVICE int64
 * step counter that this call increments before the update (so a captured
 * graph replays correct bias corrections).  The update and the increment are
 * one launch: during it the upper 32 bits hold a completion ticket, so between
 * calls *step is the plain step count and must stay below 2^32.  The gradient is multiplied by
 * grad_scale first (1/world_size after a SUM all-reduce, else 1). */
int vqhmm_adam_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   double lr, double beta1, double beta2, double eps, int64_t* step, float grad_scale,
                   void* stream);

/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) over the flat gradient
 * (Trainer.train_epoch, src/training/trainer.py:32): grad *= pre_scale, then
 * total = ||grad||_2 and grad *= min(max_norm / (total + 1e-6), 1), all on the
 * device.  total_norm (nullable, device fp32) receives the norm, which is what
 * clip_grad_norm_ returns.  pre_scale folds the 1/world of a SUM all-reduce in
 * before the norm.  Follow with vqhmm_adam_f32(..., grad_scale = 1). */
int vqhmm_clip_grad_norm_f32(float* grad, int64_t n, float pre_scale, float max_norm, float* total_norm,
                             void* stream);

/* ---------------------------------------------------------- data step ----
 * RandomChunkDataset.__getitem__ (:25-29) + collate_fn (:164-179) on the
 * device: out (B, C, Tmax) = zero-padded chunks, out[i,c,t] = t < L_i ?
 * src[base_i + c*n_i + s_i + t] : 0, with meta (B x 4 int64, device) =
 * {base_i, n_i, s_i, L_i} per sample (a row-major (C, n_i) sequence at element
 * base_i of src, chunk start s_i, length L_i).  Bit-identical to collate_fn. */
int vqhmm_gather_chunks_f32(const float* src, const int64_t* meta, int64_t B, int64_t C, int64_t Tmax,
                            float* out, void* stream);

/* ---------------------------------------------------------- inference ----
 * VAE_HMM.encode (:100, Encoder.forward :38-41): x (B,D,T) -> logits (B,K,T)
 * VAE_HMM.decode (:103, Decoder.forward :81-90): q (B,K,T) -> mu, logvar (B,D,T)
 * VAE_HMM.forward (:139-143): x -> mu, logvar, q = softmax(logits, dim=1)
 * Prior.forward (:59-71): u -> log_pi (K), log_A (B,T,K,K)
 * Unused parameter pointers may be NULL (e.g. encode needs only the encoder's). */
int vqhmm_infer_workspace_size(const vqhmm_dims_t* dims, int64_t B, int64_t T, size_t* bytes);
int vqhmm_encode_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                     int64_t B, int64_t T, float* logits, void* workspace, size_t ws_bytes, void* stream);
int vqhmm_decode_f32(const vqhmm_dims_t* dims, const float* const* params, const float* q,
                     int64_t B, int64_t T, float* mu, float* logvar, void* workspace, size_t ws_bytes,
                     void* stream);
int vqhmm_forward_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                      int64_t B, int64_t T, float* mu, float* logvar, float* q, void* workspace,
                      size_t ws_bytes, void* stream);
int vqhmm_prior_f32(const vqhmm_dims_t* dims, const float* const* params, const float* u, int u_layout,
                    int64_t B, int64_t T, float* log_pi, float* log_A, void* stream);
/* Autograd of the module surface (VAE_HMM.encode / decode / forward under torch autograd, :100-104,
 * :139-143; examples/backtest_example.py:30 calls encode with grad enabled).  Each recomputes its module's
 * forward into the workspace (vqhmm_module_bwd_workspace_size), then runs the data gradients, the weight
 * gradients and one fixed-order slab reduction.  grad: the flat buffer of vqhmm_param_layout(dims); only the
 * module's own entries are written (encode: encoder.*; decode: decoder.*; forward: both).  Output gradients
 * are channels-first like the outputs: dlogits (B,K,T); dpar = [dmu | dlogvar] (B,2D,T); dq (B,K,T) the
 * gradient of forward's q output (NULL: 0; forward's dpar NULL: 0).  Input gradients dx (B,D,T) / dq (B,K,T)
 * are written when non-NULL. */
int vqhmm_module_bwd_workspace_size(const vqhmm_dims_t* dims, int64_t B, int64_t T, size_t* bytes);
int vqhmm_encode_bwd_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                         const float* dlogits, int64_t B, int64_t T, void* workspace, size_t ws_bytes,
                         float* grad, float* dx, void* stream);
int vqhmm_decode_bwd_f32(const vqhmm_dims_t* dims, const float* const* params, const float* q,
                         const float* dpar, int64_t B, int64_t T, void* workspace, size_t ws_bytes,
                         float* grad, float* dq, void* stream);
int vqhmm_forward_bwd_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x,
                          const float* dpar, const float* dq, int64_t B, int64_t T, void* workspace,
                          size_t ws_bytes, float* grad, float* dx, void* stream);
/* Autograd of Prior.forward (VQ_VAE_HMM_fixed.py:59-71) alone: dlog_pi (K, nullable = 0) and dlog_A
 * (B,T,K,K) -> grad's prior.* entries (log_prior, transition_net.0/.2 weight and bias; nothing else is
 * written) and du (nullable; CF (B, U, T) whatever u_layout).  Recomputes the MLP into the workspace
 * (vqhmm_prior_bwd_workspace_size), then the log_softmax backwards, the hidden layer's masked data
 * gradient, du, the two weight gradients and one fixed-order slab reduction. */
int vqhmm_prior_bwd_workspace_size(const vqhmm_dims_t* dims, int64_t B, int64_t T, size_t* bytes);
int vqhmm_prior_bwd_f32(const vqhmm_dims_t* dims, const float* const* params, const float* u, int u_layout,
                        const float* dlog_pi, const float* dlog_A, int64_t B, int64_t T, void* workspace,
                        size_t ws_bytes, float* grad, float* du, void* stream);

/* ------------------------------------------- fused Prior -> Viterbi ----
 * the Viterbi path of vqhmm_viterbi_f32 over the tables vqhmm_prior_f32 would write
 * (Prior.forward VQ_VAE_HMM_fixed.py:59-71), computed per chunk on the chip from u and never stored:
 * HBM reads u (4U B per position) instead of log_A (4K^2 B, written then read).  u as in
 * vqhmm_prior_f32 (u_layout 0: (B,U,T), 1: (B,T,U)); em (B,T,K); lengths (B) int64 ->
 * path (B,T) int32, score (B).  path / score equal vqhmm_viterbi_f32 on vqhmm_prior_f32's log_pi and
 * log_A bit for bit.  K <= 8, u_dim <= 4, trans_hidden in {64, 128, 256}; other dims ->
 * VQHMM_EUNSUPPORTED (run vqhmm_prior_f32 + vqhmm_viterbi_f32).  Workspace:
 * vqhmm_prior_viterbi_workspace_size(dims, B, T) bytes. */
size_t vqhmm_prior_viterbi_workspace_size(const vqhmm_dims_t* dims, int64_t B, int64_t T);
int vqhmm_prior_viterbi_f32(const vqhmm_dims_t* dims, const float* const* params, const float* u, int u_layout,
                            const float* em, const int64_t* lengths, int64_t B, int64_t T, int32_t* path,
                            float* score, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------- hard regimes ----
 * regime_probs.argmax(dim=1) of softmax(encode(x), dim=1) — backtesting.py:154-155,
 * src/backtesting.py:105-107, VQ_VAE+HMM.ipynb:830, visualize.ipynb:74.  One fused
 * pass: the encoder's to_logits epilogue computes q and its first argmax.
 * x (B,D,T) -> regimes (B,T) int32 and, if q != NULL, q (B,K,T) fp32 (the probabilities
 * the argmax was taken over).  Argmax rule = torch.argmax: NaN is the maximum, the
 * lowest index wins ties; so regimes == q.argmax(dim=1) bit for bit.  Workspace:
 * vqhmm_infer_workspace_size. */
int vqhmm_regimes_f32(const vqhmm_dims_t* dims, const float* const* params, const float* x, int64_t B, int64_t T,
                      float* q, int32_t* regimes, void* workspace, size_t ws_bytes, void* stream);
/* Same argmax rule over the channel axis of any CF tensor: q (B,K,T) -> idx (B,T) int32. */
int vqhmm_argmax_f32(const float* q, int64_t B, int64_t K, int64_t T, int32_t* idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQHMM_H */
