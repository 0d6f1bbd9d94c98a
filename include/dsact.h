/*
 * dsact.h -- C-ABI of libdsact.so: the MI355X-native (gfx950) DSAC-T off-policy update path.
 *
 * This is the drop-in boundary for ONE path of Jingliang-Duan/DSAC-v2 (all file:line below are
 * relative to the reference repository):
 *
 *   dsac_v2.py:150-206   DSAC_V2.__compute_gradient      -> dsact_compute_grads
 *   dsac_v2.py:320-347   DSAC_V2.__update                -> dsact_apply_update
 *   dsac_v2.py:102-105   DSAC_V2.local_update            -> dsact_step
 *   dsac_v2.py:107-138   get_remote_update_info / remote_update (data-parallel seam)
 *                                                        -> dsact_compute_grads / [all-reduce of the
 *                                                           bound gradient arena] / dsact_apply_update
 *   training/replay_buffer.py:20-50   ReplayBuffer.__init__   -> dsact_buffer_create
 *   training/replay_buffer.py:58-83   store / add_batch       -> dsact_buffer_add
 *   training/replay_buffer.py:85-90   sample_batch            -> dsact_gather (index draw stays on the
 *                                                                host: np.random.randint, bit-exact;
 *                                                                opt-in device draw: dsact_set_index_rng)
 *   training/trainer.py:72-74         per-key .cuda() of a CPU minibatch -> dsact_load_batch
 *   dsac_v2.py:188-204                the 14 numeric tb_info entries     -> dsact_read_stats
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success, a negative DSACT_E_* on
 *     failure; the message of the last failure on a handle is dsact_last_error(h).
 *   - all device work is enqueued on ONE stream per handle (dsact_set_stream; default: a stream the
 *     handle owns). Calls are asynchronous unless stated; one handle is used from one host thread.
 *   - parameter / optimiser memory is OWNED BY THE CALLER (torch-ROCm tensors on the Python side):
 *     dsact_bind_arenas only records device pointers. Flat fp32 arena order:
 *         online  : q1 | q2 | policy | log_alpha        (dsact_online_count floats)
 *         target  : q1_target | q2_target | policy_target
 *         adam_m, adam_v, grads : same order and size as `online`; `grads` has 2 extra floats at the
 *                   tail (the updated mean_std1/2 EMA, so that ONE all-reduce re-synchronises them)
 *     inside a net: [W0 (out x in, row-major, == nn.Linear.weight) | b0 | W1 | b1 | ...], i.e. the
 *     parameter order of torch's state_dict.
 *     CNN nets (conv_type != 0): [conv0.w | conv0.b | ... | MLP part]. conv weights are stored
 *     [Cout][KH][KW][Cin] (torch's [Cout][Cin][KH][KW] permuted: a dense [Cout x K] matrix whose K order
 *     makes image patches contiguous). The MLP part holds the `mean` and `log_std` MLPs side by side:
 *     layer 0 = [mean.0.weight ; log_std.0.weight] stacked by rows (2H0 x in) | [b_mean ; b_ls];
 *     hidden layer l = mean.W_l (H x H) | log_std.W_l (H x H) | [b_mean ; b_ls];
 *     output layer = (n_out x 2H) matrix [[w_mean, 0], [0, w_ls]] (the zero blocks are structural:
 *     never written by the gradient path, never changed by Adam) | [b_mean ; b_ls].
 *   - all tensors fp32; replay indices int64 on the host API (int32 on device).
 */
#ifndef DSACT_H
#define DSACT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSACT_MAX_HIDDEN_LAYERS 6
#define DSACT_ALGO_DSAC_V2 0
#define DSACT_ALGO_DSAC_V1 1
#define DSACT_CONV_NONE 0
#define DSACT_CONV_TYPE_1 1
#define DSACT_CONV_TYPE_2 2

#define DSACT_OK 0
#define DSACT_E_INVALID (-1)   /* bad argument / unsupported configuration */
#define DSACT_E_HIP (-2)       /* a HIP runtime call failed */
#define DSACT_E_STATE (-3)     /* call order violated (arenas not bound, buffer empty, ...) */
#define DSACT_E_NODEVICE (-4)  /* no MI355X visible */

typedef struct dsact_handle dsact_handle;

/* Hyper-parameters consumed by DSAC_V2.__init__ / ApproxContainer.__init__
 * (dsac_v2.py:27-59,81-90; utils/common_utils.py:48-89). */
typedef struct dsact_config {
  int32_t obs_dim;                              /* obsv_dim */
  int32_t act_dim;                              /* action_dim (<= 32) */
  int32_t n_hidden;                             /* len(hidden_sizes), 1..DSACT_MAX_HIDDEN_LAYERS */
  int32_t hidden[DSACT_MAX_HIDDEN_LAYERS];      /* value/policy_hidden_sizes (same for both) */
  int32_t batch;                                /* replay_batch_size (local batch of this rank) */
  int32_t global_batch;                         /* batch summed over data-parallel ranks (>= batch) */
  int32_t auto_alpha;                           /* auto_alpha */
  int32_t delay_update;                         /* delay_update */
  /* Hyper-parameters cross the boundary as the Python doubles the reference holds: torch.optim.Adam computes its
   * step size and bias corrections, and dsac_v2.py:331 its Polyak factor, in double arithmetic before touching an
   * fp32 tensor -- so does this library, for any value (not only short decimals). */
  double gamma, tau, tau_b;                     /* gamma, tau, tau_b (= tau when absent) */
  double lr_q, lr_pi, lr_alpha;                 /* value/policy/alpha_learning_rate */
  double alpha_fixed;                           /* alpha when !auto_alpha */
  double min_log_std, max_log_std;              /* policy_min/max_log_std */
  double adam_beta1, adam_beta2, adam_eps;      /* torch.optim.Adam defaults 0.9, 0.999, 1e-8 */
  /* CNN approximators (value/policy_func_type == "CNN", networks/cnn.py:151-240,383-461):
   * conv_type 0 = MLP nets; 1 = "type_1" (k 8,4,3 / ch 32,64,64 / stride 4,2,1, hidden 512,256);
   * 2 = "type_2" (k 4,3,3,3,3,3 / ch 8..256 / stride 2,2,2,2,1,1, hidden 256,256,256).
   * With conv_type != 0: obs_dim = img_c*img_h*img_w (replay rows hold the (C,H,W) image), `hidden`
   * are the widths of the `mean` / `log_std` MLPs that follow the conv stack. */
  int32_t conv_type;
  int32_t img_c, img_h, img_w;
  /* algo 0 = DSAC_V2 (DSAC-T: twin critics, mean_std refinements); 1 = DSAC_V1 (reference dsac_v1.py: ONE critic
   * `q` + `q_target`, fixed TD_bound, variance-weighted critic pseudo-loss :217-226). With algo 1 the arenas are
   * online = q | policy | log_alpha and target = q_target | policy_target; MLP nets only. */
  int32_t algo;
  double td_bound;                              /* TD_bound (DSAC_V1 only; reference default 20) */
  int32_t v1_unbounded;                         /* DSAC_V1 `bound` kwarg NEGATED (0 = the reference default bound=True, the
                                                 * variance-weighted pseudo-loss of dsac_v1.py:217-226; 1 = bound=False, the plain
                                                 * Gaussian negative log-likelihood of :227-228) */
  /* value_hidden_activation / policy_hidden_activation (utils/common_utils.py:16-45): 0 gelu (every shipped example),
   * 1 relu, 2 elu, 3 selu, 4 sigmoid, 5 tanh -- torch's default arguments. Output activations are linear. */
  int32_t value_act, policy_act;
  /* policy_act_distribution (utils/act_distribution_cls.py): 0 = "TanhGaussDistribution" (:21-79, every shipped example),
   * 1 = "GaussDistribution" (:82-115: no squashing -- action = mean + std * eps, log-prob of the plain diagonal Gaussian;
   * the action limits are only used by the caller's clipping and by mode()). */
  int32_t act_dist;
  /* policy_std_type (networks/mlp.py:43-73): 0 = "mlp_shared" (one MLP -> mean | log_std; every shipped example),
   * 1 = "parameter" (:63-73,92-97: the MLP gives the mean, log_std is a learnable (1, act_dim) parameter). With 1 the arenas
   * keep the (2 act_dim x H) output layer: rows [act_dim, 2 act_dim) of its weight are structurally zero (the caller zeroes
   * them once; their gradient is masked, so Adam / Polyak leave them at 0) and the second half of its bias IS log_std.
   * DSAC_V2 with MLP nets, on BOTH kernel families: the row-slice chains (equal hidden widths 64 / 128 / 256, batch a multiple
   * of 16; DwProb::msplit masks the gradient) and the tile stages (every other shape, incl. split-K at batch > 448, unequal
   * widths and non-linear output activations; GemmProb::mzero) -- tests/test_std_parameter.py covers a shape of each. */
  int32_t policy_std_param;
  /* value_output_activation / policy_output_activation (utils/common_utils.py:16-45 -> networks/mlp.py:15-20: the module that
   * follows the LAST Linear): 0 = "linear" (every shipped example), 1 relu, 2 elu, 3 selu, 4 sigmoid, 5 tanh, 6 gelu (whose
   * derivative is no function of its output: the tile-stage heads store it beside the output, and a handle with it stays on the
   * tile-stage kernels). DSAC_V2 with MLP nets only. Round 6: served by the row-slice chains wherever a linear head would
   * be (the generic-activation instantiations of the forward kernels apply it in the heads, the backward row phases multiply by
   * its derivative expressed through the stored POST-activation outputs) and by both acting forwards; shapes the chains do not
   * take, and batch >= 1024's throughput-regime kernels, fall to the chains' generic forms / the tile-stage kernels as for linear
   * heads. With policy_std_param the policy's activation applies to the mean half only (log_std is a plain parameter,
   * networks/mlp.py:92-97). */
  int32_t value_out_act, policy_out_act;
  /* value_hidden_sizes != policy_hidden_sizes (utils/common_utils.py:59-62 reads them per key): `hidden` sizes the critics,
   * `policy_hidden[l]` > 0 the policy nets (all zeros: the same widths); policy_n_hidden below for another number of layers.
   * DSAC_V2 with MLP nets on the tile-stage kernels (the row-slice chains run one width per layer across every unit -- a caller
   * who wants such nets on the chains stores them zero-padded to a common width and passes THAT as `hidden`: the Python host
   * side does, dsac-v2_amd/dsact/layout.py ArenaLayout pad_to). */
  int32_t policy_hidden[DSACT_MAX_HIDDEN_LAYERS];
  /* policy_std_type "mlp_separated" (networks/mlp.py:46-57,80-85): 1 = the policy is TWO MLPs over the observation, `mean` and
   * `log_std`, each obs -> hidden -> act_dim (0: one of the two forms policy_std_param selects). The arenas keep them side by
   * side, exactly as the CNN nets' twin trunks: layer 0 one dense (2 H0 x obs) matrix [mean.0 ; log_std.0], hidden layer l two
   * (H x Hprev) blocks mean | log_std, output layer the dense (2 act_dim x 2 H) matrix [[w_mean, 0], [0, w_log_std]] whose two
   * zero blocks are structural (the caller zeroes them once; no gradient is ever written there), biases [b_mean ; b_log_std].
   * DSAC_V2 with MLP nets, tile-stage kernels (the critics stay single MLPs: the row-slice chains run one trunk count per
   * launch); policy_std_param must be 0. Both acting forwards serve it (a block layer is a row range with an input offset). */
  int32_t policy_twin;
  /* len(policy_hidden_sizes) when it differs from len(value_hidden_sizes) (0: the same number of layers). The policy nets then
   * take `policy_hidden[0 .. policy_n_hidden)` (every entry > 0) and their own depth everywhere; the critics keep `n_hidden` /
   * `hidden`. DSAC_V2 with MLP nets, tile-stage kernels (stage lists, heads and weight-gradient tiles are built per net). */
  int32_t policy_n_hidden;
} dsact_config;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int dsact_version(void);
int dsact_device_count(void);
int dsact_create(const dsact_config* cfg, int device, dsact_handle** out);
int dsact_destroy(dsact_handle* h);
const char* dsact_last_error(const dsact_handle* h);
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL -> handle-owned stream */
int dsact_set_stream(dsact_handle* h, void* hip_stream);
/* the hipStream_t every call on this handle enqueues on -- host code that interleaves its own device work
 * (torch.distributed collectives on the gradient arena, dsac_v2.py:107-138 seam) must issue it on THIS stream
 * (torch.cuda.ExternalStream) or order against it with events; never NULL after dsact_create */
void* dsact_get_stream(const dsact_handle* h);
int dsact_sync(dsact_handle* h); /* blocks until the handle's stream is idle */

/* ---- parameters (ApproxContainer, dsac_v2.py:19-62) ------------------------------------------- */
size_t dsact_online_count(const dsact_handle* h); /* floats in q1|q2|policy|log_alpha */
size_t dsact_target_count(const dsact_handle* h); /* floats in q1_t|q2_t|policy_t */
size_t dsact_q_count(const dsact_handle* h);      /* floats in one Q net */
size_t dsact_pi_count(const dsact_handle* h);     /* floats in the policy net */
int dsact_bind_arenas(dsact_handle* h, float* online, float* target, float* adam_m, float* adam_v,
                      float* grads /* online_count + 2 floats */);
/* act_high_lim / act_low_lim buffers of StochaPolicy (networks/mlp.py:75-76); host pointers */
int dsact_set_action_limits(dsact_handle* h, const float* high, const float* low);
/* Adam step counters (q, policy, alpha) and the mean_std EMA state (dsac_v2.py:88-89,233-241);
 * mean_std < 0 encodes the reference's -1.0 "not yet initialised" sentinel. Synchronous.
 * dsact_set_state (and a successful dsact_bind_arenas) also ACKNOWLEDGES a hand-over timeout: after one (DSACT_E_HIP from
 * any entry point, see dsact_debug_set below) parameters / moments / targets are suspect and every update entry point
 * fails with DSACT_E_STATE until the caller has restored them and called one of the two
 * (dsact_debug_get(h, "state_invalid") reads the flag). */
int dsact_get_state(dsact_handle* h, int32_t adam_steps[3], float mean_std[2]);
int dsact_set_state(dsact_handle* h, const int32_t adam_steps[3], const float mean_std[2]);
/* The reference re-reads its `adjustable_parameters` (dsac_v2.py:92-99: gamma, tau, auto_alpha, alpha, delay_update;
 * dsac_v1.py adds TD_bound) on every update, so assigning one between updates takes effect on the next. Same here:
 * the value is used from the next enqueued update on; a captured graph (dsact_graph_build) has the old value baked
 * in and is dropped -- build it again. tau also sets tau_b when `also_tau_b` semantics apply (DSACT_HYPER_TAU keeps
 * tau_b untouched; set DSACT_HYPER_TAU_B explicitly). */
#define DSACT_HYPER_GAMMA 0
#define DSACT_HYPER_TAU 1
#define DSACT_HYPER_TAU_B 2
#define DSACT_HYPER_AUTO_ALPHA 3
#define DSACT_HYPER_ALPHA 4
#define DSACT_HYPER_DELAY_UPDATE 5
#define DSACT_HYPER_V1_BOUND 7      /* DSAC_V1 `bound` (0 / 1) */
#define DSACT_HYPER_TD_BOUND 6
int dsact_set_hyper(dsact_handle* h, int32_t which, double value);

/* ---- replay buffer (training/replay_buffer.py) -------------------------------------------------- */
int dsact_buffer_create(dsact_handle* h, int64_t capacity);
/* n transitions, SoA host arrays (obs[n*O], act[n*A], rew[n], obs2[n*O], done[n], logp[n]); ring
 * write at ptr with the reference's ptr/size semantics (replay_buffer.py:58-79). ASYNCHRONOUS: the arrays are copied
 * into a pinned staging slot before the call returns (the caller may reuse them at once), one H2D copy and the ring
 * write are enqueued on the handle's stream and nothing waits for them; every later call on the handle is ordered
 * behind them. dsact_buffer_size / dsact_buffer_ptr reflect the add immediately. */
int dsact_buffer_add(dsact_handle* h, int64_t n, const float* obs, const float* act, const float* rew,
                     const float* obs2, const float* done, const float* logp);
int64_t dsact_buffer_size(const dsact_handle* h);
int64_t dsact_buffer_ptr(const dsact_handle* h);
/* bulk fill of rows [row0,row0+n) directly from DEVICE arrays (synthetic benchmark buffers);
 * sets size=max(size,row0+n), ptr=(row0+n)%capacity */
int dsact_buffer_fill_device(dsact_handle* h, int64_t row0, int64_t n, const float* obs, const float* act,
                             const float* rew, const float* obs2, const float* done);
/* Coded image ring (CNN handles only; H*W % 16 == 0, C <= 16): instead of dsact_buffer_create. The obs / obs2 columns hold
 * one byte per element, an index into codebook[0..n_codes) -- at most 256 float32 values, strictly ascending (no NaN, no
 * duplicates, not both -0.0 and 0.0). dsact_buffer_add and dsact_buffer_fill_device still take fp32 rows and encode them
 * on the device; a value matches an entry only if its bits are equal, so every stored value comes back bit for bit and
 * everything downstream equals the fp32 ring. A value missing from the table is never rounded silently: the encoder counts
 * it and records the first one seen, and every call on the handle that starts after that write has completed on the
 * device (add, fill, gather, step, graph, group, data-parallel enqueues) fails with DSACT_E_INVALID naming it, as does
 * dsact_buffer_check. Rows never written hold code 0. */
int dsact_buffer_create_coded(dsact_handle* h, int64_t capacity, const float* codebook, int32_t n_codes);
/* SYNCHRONOUS: drains the stream, then DSACT_E_INVALID if a value missing from the codebook was written (OK for fp32 rings) */
int dsact_buffer_check(dsact_handle* h);
/* device bytes of the ring: capacity * (2*O + 4*(A+3)) coded, capacity * 4*(2*O + A + 3) fp32; 0 before a create */
int64_t dsact_buffer_bytes(const dsact_handle* h);
/* Ring snapshots (training/hip_replay_buffer.py save / load): the ring's STORED FORM out of and into HBM,
 * its cursor, and an integrity digest computed on the device. Stored form, per column in the SoA order obs, obs2, act, rew,
 * done, logp: obs / obs2 float32[O] per row on an fp32 ring, uint8[O] codes per row on a coded ring; act float32[A]; rew, done
 * and logp one float32 each. All four calls are SYNCHRONOUS: every argument is validated on the host before any launch or
 * copy, the handle's stream is drained first, and the call returns with its work complete. DSACT_E_STATE before a ring was
 * created or under stream capture.
 *   dsact_buffer_export      copies ring rows [row0, row0 + n) to HOST arrays in stored form (each column's slice is
 *                            contiguous in the ring: plain copies, no kernel); any destination may be NULL. 0 <= row0, 0 <= n,
 *                            row0 + n <= size (DSACT_E_INVALID otherwise); n == 0 is a no-op.
 *   dsact_buffer_import      writes ring rows [row0, row0 + n) from HOST arrays in stored form, none NULL; row0 + n <= capacity.
 *                            Moves neither size nor ptr. On a coded ring every code must be < n_codes: checked on the host
 *                            before the first byte is uploaded -- a refused import leaves the ring untouched.
 *   dsact_buffer_set_cursor  sets size and ptr to a state replay_buffer.py:58-79 reaches: 0 <= size <= capacity, and
 *                            ptr == size % capacity while size < capacity, 0 <= ptr < capacity when size == capacity
 *                            (DSACT_E_INVALID otherwise).
 *   dsact_buffer_digest      six 64-bit sums, one per column c = 0..5 (obs, obs2, act, rew, done, logp; widths w_c = O, O, A,
 *                            1, 1, 1), over rows [row0, row0 + n), row0 + n <= size, computed on the device from the stored
 *                            bits (k_ring_digest). Not cryptographic: it tells whether what reached HBM is what was saved, and
 *                            compares two rings bit for bit without moving them to the host. For the element at ring row r,
 *                            position j: g = r * w_c + j as a 64-bit integer, v = the stored value's bits zero-extended (the
 *                            float's 32 bits, or the code byte), and with all arithmetic mod 2^64
 *                                x = g * 0x9E3779B97F4A7C15 + (((uint64)(c + 1) << 32) | v)
 *                                x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *                                out[c] = sum of x over the column's elements in the row range
 *                            An integer sum: independent of the order of addition, and the digest of a range is the sum of
 *                            the digests of its parts. g uses the ABSOLUTE ring row: the same row written at another position
 *                            digests differently. n == 0 gives six zeros. */
int dsact_buffer_export(dsact_handle* h, int64_t row0, int64_t n, void* obs, void* obs2, float* act, float* rew, float* done,
                        float* logp);
int dsact_buffer_import(dsact_handle* h, int64_t row0, int64_t n, const void* obs, const void* obs2, const float* act,
                        const float* rew, const float* done, const float* logp);
int dsact_buffer_set_cursor(dsact_handle* h, int64_t size, int64_t ptr);
int dsact_buffer_digest(dsact_handle* h, int64_t row0, int64_t n, uint64_t out[6]);
/* Background snapshots (training/hip_replay_buffer.py save_async): a consistent copy of the live rows is
 * taken INSIDE HBM in stream order -- one launch (k_ring_shadow) copies rows [0, size) of the six columns into a library-owned
 * "shadow" with the same SoA order and stored form, and digests every chunk of chunk_rows rows over the same bytes -- and a
 * second host thread moves the shadow to the host while the owning thread goes on issuing work on the handle.
 *
 * WHICH THREAD CALLS WHAT. The OWNING thread is the one that makes every other call on the handle; it alone calls take and
 * release. ONE OTHER thread (the reader) may call export, digests and error between a take and its release, concurrently with
 * anything the owning thread does on the handle. The two share one small struct behind a mutex and nothing else: the reader
 * calls never touch the handle's stream, its hand-over words, its graph cache or the text of dsact_last_error.
 *   take     (owning thread) stream-ordered, NEVER waits: validates, grows the shadow and digest allocations if needed (an
 *            allocation it replaces is kept until the next release: freeing waits for the device), zeroes the digests,
 *            launches k_ring_shadow on the handle's stream and records an event behind it. What it captured -- size, ptr,
 *            chunk_rows, n_chunks = ceil(size / chunk_rows) and bytes (the padded columns of `size` rows plus 48 bytes per
 *            chunk) -- is remembered and returned in *info_out. Rows written to the ring after the call do not reach the
 *            shadow. Refused before anything is allocated or enqueued: DSACT_E_STATE without a ring, under stream capture,
 *            or while a shadow is taken and not released; DSACT_E_INVALID for chunk_rows < 1 or bytes > max_bytes (0: no
 *            bound). An empty ring gives an empty shadow with n_chunks = 0. A first take allocates for the ring's CAPACITY
 *            when max_bytes allows it, so that a ring that is still filling does not grow its shadow again.
 *   export   (reader) rows [row0, row0 + n) of the shadow to HOST arrays, as the synchronous export does from the ring: any
 *            destination may be NULL, 0 <= row0, 0 <= n, row0 + n <= the size TAKEN. Waits for the take's event only, copies on
 *            a private copy stream and synchronises that stream only.
 *   digests  (reader) out[n_chunks][6]: word [k][c] equals what the synchronous digest of rows [k * chunk_rows, + rows of
 *            chunk k) gave for column c at the take. n_chunks must be the take's.
 *   error    (reader) the text of the reader calls' last failure (they return the same codes as every other call).
 *   release  (owning thread, after the reader is done; DSACT_E_STATE while a reader call runs) marks the shadow free for the
 *            next take; free_memory != 0 also frees its device memory (that waits for the device). The destroy call
 *            synchronises the copy stream and frees whatever is left.
 * dsact_debug_get: "shadow_state" (1 between take and release), "shadow_bytes" (device bytes allocated), "shadow_takes". */
typedef struct dsact_shadow_info {
  int64_t size, ptr, chunk_rows, n_chunks;
  uint64_t bytes;
} dsact_shadow_info;
int dsact_buffer_shadow_take(dsact_handle* h, int64_t chunk_rows, uint64_t max_bytes, dsact_shadow_info* info_out);
int dsact_buffer_shadow_export(dsact_handle* h, int64_t row0, int64_t n, void* obs, void* obs2, float* act, float* rew, float* done,
                               float* logp);
int dsact_buffer_shadow_digests(dsact_handle* h, uint64_t* out, int64_t n_chunks);
const char* dsact_buffer_shadow_error(const dsact_handle* h);
int dsact_buffer_shadow_release(dsact_handle* h, int32_t free_memory);
/* gather rows idx[0..batch) into the handle's minibatch staging area (== sample_batch + .cuda()). idx_host == NULL (an
 * index seed is set, DSACT_E_STATE otherwise): the rows of index-table row 0 as dsact_draw_indices left it, copied device to
 * device behind the draw -- replay_buffer.py:86-90 with no host index at all. */
int dsact_gather(dsact_handle* h, const int64_t* idx_host, int32_t batch);
/* copy the staged minibatch back to host arrays (any may be NULL); synchronous. `logp` comes from
 * the ring (it is not part of the staging area the update reads). */
int dsact_read_batch(dsact_handle* h, float* obs, float* act, float* rew, float* obs2, float* done,
                     float* logp);
/* stage a minibatch produced elsewhere (reference ReplayBuffer + new algorithm mix). Each pointer may be a HOST
 * array (the reference's CPU batch) or a DEVICE array on the handle's GPU (the reference trainer's `.cuda()`
 * tensors, training/trainer.py:72-74: no round trip through the host); the copies are issued on the handle's
 * stream and completed before the call returns, so the caller must have finished writing the sources. */
int dsact_load_batch(dsact_handle* h, const float* obs, const float* act, const float* rew,
                     const float* obs2, const float* done);
/* index table for graph replay: rows x batch indices, row r is consumed by the r-th replayed step */
int dsact_upload_index_table(dsact_handle* h, const int64_t* idx_host, int32_t rows);

/* Device-side index draw (opt-in; replaces the np.random.randint(0, size, batch) of replay_buffer.py:86 the caller otherwise
 * makes on the host). Every update's `batch` indices are drawn uniformly with replacement in [0, size) from Philox4x32-10
 * with counter (position / 2, iteration low, iteration high, stream id 4) and key = seed (low, high word); the noise of
 * dsact_set_device_rng uses stream ids 1 .. 3 of the same generator, so the two never share a counter block whatever their
 * seeds. One Philox call gives words w[0..3] = two 64-bit draws u_k = (w[2k+1] << 32) | w[2k] for positions 2p + k, and
 * index = floor(u * size / 2^64) (the high 64 bits of the 128-bit product). That map is a pure function of (seed, iteration,
 * position, size); its bias is at most size / 2^64 per index (below 2^-40 for a 10M-row ring), it is not exactly uniform.
 * The values depend on the iteration, never on the grouping: row r of a draw starting at iteration i is the one-row draw
 * at i + r. A run is reproducible from its seeds; it is NOT index for index the reference's run (the NumPy stream is not
 * consumed), exactly as dsact_set_device_rng's noise is not torch.randn's.
 *   dsact_set_index_rng(h, seed)   0 disables (the default). Independent of dsact_set_device_rng; not baked into any graph.
 *   dsact_draw_indices(h, first_iteration, n)   replay_buffer.py:86 for n consecutive updates without an update: enqueues
 *                                  the draw over the ring size at the time of the call; afterwards rows [0, n) of the
 *                                  index table hold it (for dsact_gather(h, NULL, batch), data-parallel replays that
 *                                  read the table, and tests). DSACT_E_STATE without a seed or on an empty ring
 *                                  (np.random.randint(0, 0) raises too). Asynchronous.
 *   dsact_read_indices(h, out, rows)   the first `rows` index-table rows as int64 out[rows * batch] -- what
 *                                  replay_buffer.py:86 returned for them. SYNCHRONOUS (tokens that must re-gather, tests). */
int dsact_set_index_rng(dsact_handle* h, uint64_t seed);
int dsact_draw_indices(dsact_handle* h, int64_t first_iteration, int32_t n);
int dsact_read_indices(dsact_handle* h, int64_t* out, int32_t rows);

/* ---- noise (the torch.randn draws of one __compute_gradient) ------------- */
/* parity mode: inject eps_new[B*A], eps_2[B*A], z5[B], z6[B] (host pointers) for the next step */
int dsact_set_noise(dsact_handle* h, const float* eps_new, const float* eps_2, const float* z5,
                    const float* z6);
/* production mode: device Philox4x32-10 + Box-Muller keyed by (seed, iteration); 0 disables.
 * Every update's eps_new, eps_2, z5 and z6 are drawn where its minibatch is staged (the prologue of dsact_compute_grads /
 * dsact_step, the gathers and their riders in graph replays) as a pure function of (seed, iteration, row, action dimension):
 *   words    Philox4x32-10, counter (index, iteration low, iteration high, stream id), key = seed (low, high word)
 *   eps_new  stream id 1, eps_2 stream id 2: element [row][d] is normal d % 4 of the call with index row * ceil(A / 4) + d / 4
 *            (a row's last call is used in part when A % 4 != 0; no call serves two rows)
 *   z5 | z6  stream id 3, index row: z5[row] is normal 0, z6[row] normal 1 of the call (normals 2 and 3 are not used)
 *   map      u_k = ((float)(w[k] >> 8) + 0.5f) * 2^-24 in fp32 (the add rounds to even once w >> 8 >= 2^23, so the largest u is
 *            1.0 and its normals are 0); r(u) = sqrt(-2 ln u); normals 0, 1 = r(u_0) (cos, sin)(2 pi u_1), normals 2, 3 =
 *            r(u_2) (cos, sin)(2 pi u_3), all in fp32. |normal| <= r(2^-25) = 5.89.
 * Stream ids 4 (dsact_set_index_rng) and 5 (dsact_set_act_rng) belong to the index draw and the acting noise, 6 to the
 * exploration noise (dsact_set_explore_noise).
 * tests/noise_reference.py restates this; tests/test_update_noise_gpu.py holds every drawing site to it. */
int dsact_set_device_rng(dsact_handle* h, uint64_t seed);

/* ---- the update ----------------------------------------------------------------------------------- */
#define DSACT_F_DATA_PARALLEL 2u           /* dsact_graph_build: capture gather -> grads -> all-reduce (dsact_comm_init) -> apply */
#define DSACT_F_SKIP_ACTOR_ON_OFF_ITERS 1u /* "fast": skip actor/alpha backward when it % delay != 0
                                              (their gradients are discarded by the reference,
                                              dsac_v2.py:174-186 vs :324); parameter trajectory is
                                              unchanged */
int dsact_compute_grads(dsact_handle* h, int64_t iteration, uint32_t flags);
int dsact_apply_update(dsact_handle* h, int64_t iteration);
int dsact_step(dsact_handle* h, int64_t iteration, uint32_t flags); /* compute_grads + apply_update */
/* hipGraph path: captures `steps_per_graph` consecutive updates (gather from the index table +
 * step, iteration read from device state) and replays them; dsact_graph_run enqueues n_steps
 * updates starting at `first_iteration` (n_steps % steps_per_graph == 0). The replay ring must not
 * be written while a graph runs: inside a graph the minibatch of update s+1 is gathered while
 * update s is still in flight (it rides in that update's loss launch); results are bit-identical
 * to the same updates issued one by one. The last update's minibatch stays staged.
 * Pipelined graph (row-slice chains, batch <= 256, device RNG or dsact_run_group's noise table, 2 <= delay_update <= 4,
 * steps_per_graph >= 2; DSACT_F_SKIP_ACTOR_ON_OFF_ITERS: the same graph without the discarded policy backward):
 * policy, log_alpha and the three target nets change only when iteration % delay_update == 0 (dsac_v2.py:320-347), so
 * update it + 1 of such a window sees the policy update `it` saw -- the forward launch of update `it` also evaluates
 * policy(obs) + rsample and policy_target(obs2) for the NEXT minibatch (gathered two updates ahead) and update it + 1's
 * forward launch holds only the chains that need the fresh critics. One graph per phase first_iteration % delay_update is
 * captured; dsact_graph_run picks per replay. Same bits as eager updates. Configurations that do not meet these
 * conditions capture the plain graph; dsact_debug_get(h, "pipe_graph") tells which one was captured. */
int dsact_graph_build(dsact_handle* h, int32_t steps_per_graph, uint32_t flags);
int dsact_graph_run(dsact_handle* h, int64_t first_iteration, int64_t n_steps);
/* OffSerialTrainer.step between two sampler calls (training/trainer.py:63-82 with sample_interval = n_steps; the reference's
 * CNN examples run 8, example_train/dsacv2_cnn_carracing_offasync.py:133): n_steps x { ReplayBuffer.sample_batch
 * (replay_buffer.py:85-90) -> DSAC_V2.local_update (dsac_v2.py:102-105) } as ONE graph replay. While no add_batch intervenes
 * the ring size is constant and only np.random.randint consumes the NumPy stream (replay_buffer.py:86), so the caller
 * draws the n_steps index rows up front with the reference's own calls: idx[n_steps][batch]. noise (nullable): the
 * reference's torch.randn draws of those updates, [n_steps][2*batch*act_dim + 2*batch] floats =
 * eps_new | eps_2 | z5 | z6 per update -- strict RNG through the (pipelined) graph; NULL: device Philox keyed by the
 * iteration (dsact_set_device_rng). Asynchronous: pinned staging, a stream-ordered reset of the replay counters, no host
 * wait. Captured graphs are kept per (n_steps, flags, noise mode); the first group of a new shape pays its capture.
 * Same bits as n_steps x { dsact_gather; dsact_step }. The ring must not be written while the group runs (dsact_sync or
 * any synchronising call first) -- dsact_buffer_add is stream-ordered behind it and therefore safe.
 * idx == NULL: allowed only with an index seed (dsact_set_index_rng; DSACT_E_STATE otherwise). The n_steps draws of
 * replay_buffer.py:86 are then made by the device for iterations first_iteration .. + n_steps - 1 over the ring size at the
 * time of the call: no pinned staging, conversion or upload of index rows; one small launch on the handle's stream in front
 * of the replay, outside the captured graph (graphs and their cache keys are the same with and without it). Same bits as
 * passing dsact_read_indices' rows of the same draw as idx. With idx != NULL the call is unchanged, seed set or not. */
int dsact_run_group(dsact_handle* h, int64_t first_iteration, int32_t n_steps, const int64_t* idx, const float* noise, uint32_t flags);

/* data-parallel replay (one process per GPU): the same two halves with iteration / index-table row
 * taken from device state, so the host never touches the step. Between them the caller all-reduces
 * the bound gradient arena (online_count + 2 floats, average over ranks) on the same stream:
 *   dsact_dp_enqueue_grads  = gather(table row) + __compute_gradient   (get_remote_update_info)
 *   dsact_dp_enqueue_apply  = __update                                   (remote_update)
 * dsact_dp_begin sets the first iteration (synchronous). */
int dsact_dp_begin(dsact_handle* h, int64_t first_iteration);
int dsact_dp_enqueue_grads(dsact_handle* h, uint32_t flags);
/* dsact_dp_enqueue_grads in two halves so that the all-reduce of the critics' segment overlaps the actor's
 * backward: after _critic the q1|q2 segment of the gradient arena is final; _actor fills policy | log_alpha |
 * mean_std tail. [all_reduce(q1|q2) async] ... [all_reduce(rest)] ... dsact_dp_enqueue_apply. */
int dsact_dp_enqueue_grads_critic(dsact_handle* h, uint32_t flags);
int dsact_dp_enqueue_grads_actor(dsact_handle* h, uint32_t flags);
/* STRICT data-parallel mode: the mean_std EMA of every rank uses the GLOBAL batch
 * mean of the critics' std, which needs one 2-float all-reduce between the forward and the loss:
 *   dsact_dp_set_strict(h, buf)      buf = 2 device floats owned by the caller (a torch tensor the caller
 *                                    all-reduces with SUM); NULL switches back to the one-collective mode
 *   dsact_dp_enqueue_forward         gather + forward + local {sum std1, sum std2} -> buf
 *   [all_reduce(buf, SUM)]
 *   dsact_dp_enqueue_backward        loss (mean over cfg.global_batch) + backward -> gradient arena
 *   [all_reduce(grads) / world]      then dsact_dp_enqueue_apply as in the one-collective mode */
int dsact_dp_set_strict(dsact_handle* h, float* std_sums_dev);
int dsact_dp_enqueue_forward(dsact_handle* h, uint32_t flags);
int dsact_dp_enqueue_backward(dsact_handle* h, uint32_t flags);
int dsact_dp_enqueue_apply(dsact_handle* h);

/* ---- native collective (RCCL over xGMI) ------------------------------------------------------------------
 * The all-reduce of the data-parallel seam (dsac_v2.py:107-138: gradients out of get_remote_update_info, into
 * remote_update) issued by the library itself on the handle's stream, so that a whole data-parallel update
 * -- gather -> gradients -> all-reduce -> Adam/Polyak -- is ONE hipGraph (BASELINE.json configs[4]) with no
 * per-step host call. librccl is opened at run time (`rccl_path`: the copy torch already loaded, so that one
 * RCCL serves the process; NULL: "librccl.so").
 *   dsact_comm_unique_id   rank 0 creates the 128-byte ncclUniqueId; the caller ships it to the other ranks
 *   dsact_comm_init        every rank joins (ncclCommInitRank); the communicator lives in the handle
 *   dsact_dp_enqueue_allreduce   average of the gradient arena (+ the 2-float mean_std tail) over the ranks,
 *                          enqueued between dsact_dp_enqueue_grads and dsact_dp_enqueue_apply
 *   dsact_graph_build(..., DSACT_F_DATA_PARALLEL)  captures that chain per step; in strict mode
 *                          (dsact_dp_set_strict) also the 2-float all-reduce of the std sums before the loss */
int dsact_comm_unique_id(const char* rccl_path, uint8_t id[128]);
int dsact_comm_init(dsact_handle* h, int32_t rank, int32_t world, const uint8_t id[128], const char* rccl_path);
int dsact_comm_destroy(dsact_handle* h);
int dsact_dp_enqueue_allreduce(dsact_handle* h);

/* 14 numeric tb_info entries of the last update in the order of dsac_v2.py:188-202
 * (avg_q1, avg_q2, avg_std1, avg_std2, min_std1, min_std2, loss_actor, loss_critic, policy_mean,
 *  policy_std, entropy, alpha, mean_std1, mean_std2) + out[14] = iteration, out[15] = device milliseconds of the
 *  last dsact_step / dsact_compute_grads (stream events around it; -1 when the last update was a graph replay or a
 *  snapshot slot is read). With a gradient computed and not yet applied (dsact_compute_grads without
 *  dsact_apply_update) mean_std1/2 are the values that gradient's loss used, as the reference reports them.
 * Synchronous (this is the only per-step host sync, and only when the trainer logs). */
int dsact_read_stats(dsact_handle* h, float out[16]);
/* A reference-style caller may keep the tb_info dict of update k and read it after update k+1 has been issued
 * (deferred logging). dsact_stats_snapshot reduces the LAST update's statistics into ring slot `slot`
 * (0 .. DSACT_STATS_SLOTS-1) asynchronously -- one 64-thread launch, no host sync; dsact_stats_read copies a slot
 * out (synchronous). Same 16 floats as dsact_read_stats. */
#define DSACT_STATS_SLOTS 16
int dsact_stats_snapshot(dsact_handle* h, int32_t slot);
int dsact_stats_read(dsact_handle* h, int32_t slot, float out[16]);

/* ---- measurement / debugging -------------------------------------------------------------------- */
/* time n replays of the step on the handle's stream with hipEvents: total milliseconds */
int dsact_time_steps(dsact_handle* h, int64_t first_iteration, int64_t n_steps, uint32_t flags,
                     int32_t use_graph, float* ms_total);
/* hipEvent timing of `reps` back-to-back launches of ONE forward tile stage (k_stage<KC,KC,GELU>,
 * stage index 0..2*n_hidden-1: group A layers then group B layers) on the handle's stream; also
 * returns the stage's algorithmic multiply-accumulate count. Leaves the activations of that stage
 * overwritten (measurement only). */
int dsact_time_stage(dsact_handle* h, int32_t stage, int32_t reps, float* ms_total, double* macs);
/* 1 when this handle runs the update's MLP layers as row-slice fused chains (csrc/dsact_chain.h: DSAC_V2 / DSAC_V1 with equal
 * hidden widths of 64 / 128 / 256 and batch % 16 == 0 -- MLP nets, or the twin mean / log_std trunks of the CNN nets behind
 * their conv stacks at batch <= 1024; DSACT_NO_CHAIN=1 / DSACT_NO_CHAIN_CNN=1 force the per-layer tile stages), else 0.
 * Both paths replace the same reference functions (dsac_v2.py:150-347) and fill the same debug buffers. */
int dsact_chain_active(const dsact_handle* h);
/* per-kernel hipEvent timing of ONE eager step: fills up to `cap` entries; returns count in *n */
typedef struct dsact_kernel_time {
  char name[32];
  float ms;
  int32_t blocks;
} dsact_kernel_time;
int dsact_profile_step(dsact_handle* h, int64_t iteration, uint32_t flags, dsact_kernel_time* out,
                       int32_t cap, int32_t* n);
/* the same for n_steps consecutive updates issued eagerly as the launch sequence dsact_graph_build(n_steps, flags) would
 * capture (the pipelined sequence when that is what it would capture: its forward launches are named "chain_fwd",
 * "chain_fwd+next", "chain_fwd_q", "chain_fwd_q+next" by what they hold) */
int dsact_profile_steps(dsact_handle* h, int64_t first_iteration, int32_t n_steps, uint32_t flags, dsact_kernel_time* out,
                        int32_t cap, int32_t* n);
/* copy an internal device buffer to host by name (parity tests); returns element count in *n.
 * names: see dsact_debug_names(). */
int dsact_debug_read(dsact_handle* h, const char* name, float* out, size_t cap, size_t* n);
const char* dsact_debug_names(void);
/* Test hooks for the in-launch producer/consumer hand-overs of the merged launches (no reference counterpart: the
 * reference's update is one synchronous CPU call, dsac_v2.py:102-105). A consumer workgroup waits a BOUNDED time for
 * its producers; when it gives up, the next entry point of this library fails with DSACT_E_HIP, the merged launches are
 * disabled for the handle and a captured graph is captured again without them.
 *   dsact_debug_set(h, "withhold_flag", 1|2)    1: one forward producer never raises its ready flag; 2: one slice of the
 *                                               policy backward never arrives (both force the timeout path)
 *   dsact_debug_set(h, "poison_handover", v)    fills every buffer handed from producers to consumers with v (e.g. NaN)
 *   dsact_debug_set(h, "fwd_merge", 0|1)        merged forward launch off / on (when the shape allows it)
 *   dsact_debug_set(h, "pi_merge", 0|1)         policy weight-gradient tiles inside the policy-backward launch off / on
 *   dsact_debug_get(h, "fwd_merge" | "pi_merge" | "fat" | "handoff_failures" | "graph_steps" | "pipe_graph" |
 *                      "act_launch_us" | "act_wait_us", &v) */
int dsact_debug_set(dsact_handle* h, const char* name, double value);
int dsact_debug_get(const dsact_handle* h, const char* name, double* value);
/* stand-alone fused-MLP forward of the policy net on a host batch (sampler / evaluator feed):
 * logits[n*2A] = (mean | std) exactly as StochaPolicy.forward returns (networks/mlp.py:79-100) */
int dsact_policy_forward(dsact_handle* h, const float* obs_host, int32_t n, float* logits_host);
/* OffSampler.sample()'s device work of one environment step in ONE call (training/off_sampler.py:46-54): policy(obs) on the
 * live weights + TanhGaussDistribution.sample() (utils/act_distribution_cls.py:32-42) in the output layer's epilogue, with
 * the caller's standard-normal draw eps[A] (torch.randn(1, A): it consumes the torch generator exactly as Normal.sample()
 * does, and mean + std * eps is bit for bit what Normal.sample() returns). action[A], logp[1] on the host; MLP policies
 * (DSACT_E_INVALID otherwise -- the caller then takes dsact_policy_forward and samples itself). After
 * dsact_cnn_acting_enable also CNN policies (networks/cnn.py:151-240): obs is one (C, H, W) frame and the call is
 * dsact_act_sample_batch at n = 1, bit for bit, live or held. Synchronous. */
int dsact_act_sample(dsact_handle* h, const float* obs_host, const float* eps_host, float* action_host, float* logp_host);
/* dsact_act_sample for N environments stepped in lockstep (the vectorised sampler, training/hip_vec_sampler.py): the
 * reference's per-step acting (training/off_sampler.py:46-56) for n observation rows at once -- policy(obs) on the live
 * weights, read on the handle's stream behind every enqueued update, then TanhGaussDistribution.sample() or
 * GaussDistribution.sample() (utils/act_distribution_cls.py) in the output layer's epilogue with the caller's
 * standard-normal draws eps[n*A] (row i: torch.randn(N, A)[i]). action[n*A] and logp[n] (summed over the action
 * dimensions) on the host. obs[n*O] / eps[n*A] may be host or device pointers (as for dsact_load_batch). A row's results
 * are bitwise independent of n and of its position in the batch. Any n >= 1 (chunked inside the call); MLP policies with
 * act_dim <= 32 (DSACT_E_INVALID for CNN policies that were not enabled). After dsact_cnn_acting_enable a CNN policy
 * (networks/cnn.py:151-240) is served too: obs holds n frames of O = C*H*W floats in the environment's (C, H, W) layout, and
 * per chunk of 64 frames the call makes one copy of (frames | eps), the frame ingest, the conv stack, the feature scatter,
 * the twin trunk and the sampling launch, then one stream synchronisation. Synchronous. */
int dsact_act_sample_batch(dsact_handle* h, const float* obs, int32_t n, const float* eps, float* action_host,
                           float* logp_host);
/* The evaluator's acting for N environments stepped in lockstep (training/hip_vec_evaluator.py): the reference's
 * Evaluator.run_an_episode (training/evaluator.py:50-72) acts with dist.mode() of policy(obs) -- here for n observation rows
 * at once: action[n*A] on the host, TanhGaussDistribution.mode() = half_range * tanh(mean) + center or
 * GaussDistribution.mode() = clamp(mean, low, high) (utils/act_distribution_cls.py:71-74, :110-111), with the weights of the
 * last enqueued update. The library picks the route from n: an MLP policy that acts on the host (dsact_act_sample) runs
 * the host forward per row below a measured crossover, else the batched GPU forward of dsact_act_sample_batch with the mode
 * in its output epilogue (a row's action is then bitwise independent of n and of its position; with eps = 0 it equals
 * dsact_act_sample_batch's action bit for bit). CNN policies run dsact_policy_forward's stages in chunks of 64 frames and
 * the mode on the host. obs[n*O] may be a host or (MLP) device pointer. Any n >= 1; act_dim <= 32 (DSACT_E_INVALID
 * otherwise); DSACT_E_STATE without bound arenas or action limits. Synchronous. */
int dsact_act_mode_batch(dsact_handle* h, const float* obs, int32_t n, float* action_host);
/* Behaviour policy of an overlapped trainer (training/hip_async_trainer.py): the sampler acts with the
 * policy of the previous group while the current group's updates run.
 * dsact_behaviour_hold: on the handle's stream, behind everything already enqueued, copies the policy net's n_pi floats into a
 * device buffer of the same arena layout and records an event. From then on dsact_act_sample and dsact_act_sample_batch --
 * and ONLY they -- act with that copy: they wait for that event and never for work enqueued after it (held acting runs on a
 * third, non-blocking acting stream; a handle that acts on the host copies the snapshot into a second pinned buffer there).
 * dsact_act_mode_batch and dsact_policy_forward keep acting with the live weights. A second hold replaces the snapshot;
 * dsact_bind_arenas leaves it valid (it is a copy). DSACT_E_INVALID on CNN handles without dsact_cnn_acting_enable (with it
 * the snapshot's conv weights feed the held CNN acting forward), DSACT_E_STATE under stream capture.
 * dsact_behaviour_release: back to live acting (the default).
 * dsact_stream_idle: 1 when all work enqueued on the handle's stream has completed, else 0. Never blocks. */
int dsact_behaviour_hold(dsact_handle* h);
int dsact_behaviour_release(dsact_handle* h);
int dsact_stream_idle(dsact_handle* h);
/* CNN acting, opt-in: lets dsact_act_sample_batch, dsact_act_sample and dsact_behaviour_hold serve a CNN
 * handle -- the reference's per-step acting (training/off_sampler.py:46-56) with the image policy of networks/cnn.py:151-240,
 * as a function of (weight base, stream): live on the handle's stream, held on the acting stream with the snapshot's weights.
 * Allocates the path's own buffers for 64 frames per chunk (pinned frame stage, device frames, pixel-major frames, one
 * activation buffer per conv layer, feature rows, two trunk buffers, mapped output rows): no allocation stands between a
 * held acting call and its launches, and nothing an update reads or writes is shared. dsact_policy_forward and
 * dsact_act_mode_batch are unchanged; the device-resident forms serve the handle from then on (see below). Idempotent; DSACT_E_INVALID on an MLP handle or with
 * act_dim > 32. dsact_debug_get "cnn_act" reports the state ("act_fast" is then 1). */
int dsact_cnn_acting_enable(dsact_handle* h);

/* ---- Device-resident sampling (training/hip_tensor_sampler.py) ----------------------------------------
 * For batched simulators whose observations, rewards and done flags already live on the GPU: one environment step of N
 * environments costs launches only -- nothing is copied to or from the host and nothing waits for the stream.
 *   dsact_set_act_rng(h, seed)     the acting seed: Philox key of the in-kernel N(0,1) draw of dsact_act_sample_device; 0
 *                                  switches the draw off (the default). Replaces the torch.randn behind Normal.sample() of
 *                                  training/off_sampler.py:52-54 (utils/act_distribution_cls.py:32-42) -- standard normals
 *                                  like the reference's, not the reference's stream.
 *     generator: philox4x32-10, counter (row * ceil(A/4) + d/4, step low, step high, 5), key = the seed's (low, high) words;
 *                the four words become four normals by the Box-Muller map of the update noise (u = ((w >> 8) + 0.5) / 2^24,
 *                z0 = r(u0) cos(2 pi u1), z1 = r(u0) sin(2 pi u1), z2 = r(u2) cos(2 pi u3), z3 = r(u2) sin(2 pi u3), r(u) =
 *                sqrt(-2 ln u)); action dimension d takes element d % 4. Stream id 5: the update noise uses 1 .. 3 and the index
 *                draw 4, so no seed ever shares a counter block with them. Environment row i's noise at step t is a pure
 *                function of (seed, t, i, d): independent of n and of the chunking inside the call.
 *   dsact_act_sample_device        training/off_sampler.py:46-65 for n environments: policy(obs) on the live weights +
 *                                  TanhGaussDistribution.sample() / GaussDistribution.sample() (utils/act_distribution_cls.py)
 *                                  + the clip to the action limits (off_sampler.py:62-65), with every operand on the device:
 *                                  obs[n*O] in, action[n*A] (the distribution's sample: what the replay ring stores), logp[n]
 *                                  and clipped[n*A] = min(max(action, low), high) with the limits of dsact_set_action_limits
 *                                  (what the environment receives) out. eps[n*A]: the caller's standard-normal draws, or NULL:
 *                                  drawn in the kernel for acting step `step` (DSACT_E_STATE without a seed). With the same
 *                                  eps a row's action and logp are bit for bit dsact_act_sample_batch's. Enqueued on the handle's
 *                                  stream behind every enqueued update (the live weights, like dsact_act_sample_batch's GPU
 *                                  route) -- the inputs must be ready in that stream's order. ASYNCHRONOUS: no stream
 *                                  synchronisation, no host copy. All pointers must be device memory of the handle's GPU
 *                                  (DSACT_E_INVALID otherwise). Any n >= 1 (chunked inside the call); MLP policies with
 *                                  act_dim <= 32 (DSACT_E_INVALID for CNN policies without dsact_cnn_acting_enable; with it:
 *                                  "Device-resident image environments" below).
 *   dsact_buffer_add_device        n x ReplayBuffer.store (training/replay_buffer.py:58-79) fed from device arrays, with the
 *                                  sampler's per-step bookkeeping (training/off_sampler.py:66-73) folded in: transition i goes to
 *                                  ring row (ptr + i) % capacity; rew is stored as rew * reward_scale (ONE fp32 product with
 *                                  the scale rounded to fp32: equal to the reference's double product whenever the scale is
 *                                  exactly representable in fp32); done as terminated && !truncated (a time-out is stored
 *                                  as non-terminal); terminated / truncated: one byte per transition, non-zero = set. ptr =
 *                                  (ptr + n) % capacity, size = min(size + n, capacity) (replay_buffer.py:78-79), visible to
 *                                  dsact_buffer_size / dsact_buffer_ptr at once like dsact_buffer_add's. n <= capacity.
 *                                  ASYNCHRONOUS on the handle's stream. fp32 MLP rings (DSACT_E_INVALID on coded rings and
 *                                  CNN handles without dsact_cnn_acting_enable; with it: "Device-resident image environments"
 *                                  below); device pointers of the handle's GPU only.
 *   dsact_set_explore_noise(h, mean, std, n)   GaussNoise(mean, std) of the reference's OffSampler (training/off_sampler.py:58-65,
 *                                  utils/explore_noise.py:17-23: action = action + np.random.normal(mean, std) before the clip)
 *                                  for dsact_act_sample_device and dsact_act_sample_device_u8 ONLY -- the host-returning calls,
 *                                  the mode calls and the evaluators never add noise (the host samplers add it in Python).
 *                                  n = 0: off (the default of every handle; mean / std may be NULL). n = 1: SHARED, one normal
 *                                  per (row, step) added to every action dimension (the reference with scalar parameters).
 *                                  n = act_dim: PER-DIMENSION. Any other n, a non-finite entry or std < 0: DSACT_E_INVALID.
 *                                  mean[n], std[n] are host arrays, copied into device memory of the handle's own behind
 *                                  everything enqueued (the call waits for the stream, like dsact_set_action_limits);
 *                                  DSACT_E_STATE under stream capture. With noise on, a sampling call without an acting seed
 *                                  fails with DSACT_E_STATE -- also with eps passed in: this draw is always made in the kernel.
 *     generator: the acting draw's, on stream id 6 -- philox4x32-10, counter (row * ceil(A/4) + (shared ? 0 : d/4), step low,
 *                step high, 6), key = the acting seed, the Box-Muller map above, element shared ? 0 : d % 4: a pure function
 *                of (seed, step, row, d) that never shares a counter block with eps.
 *     epilogue:  noise = fma(std[k], z, mean[k]) (k = shared ? 0 : d; ONE rounding); a = sample + noise; action = a (what the
 *                ring stores, un-clipped); clipped = min(max(a, low), high). logp is the un-noised sample's, as in the reference.
 * dsact_debug_get: "act_dev_calls" (chunks launched by dsact_act_sample_device), "ring_commit_rows" (transitions written by
 * dsact_buffer_add_device), "act_dev_syncs" (stream synchronisations made inside the two: 0), "explore_noise" (0, 1 or act_dim:
 * the n of the last dsact_set_explore_noise). */
int dsact_set_act_rng(dsact_handle* h, uint64_t seed);
int dsact_set_explore_noise(dsact_handle* h, const float* mean, const float* std, int32_t n);
int dsact_act_sample_device(dsact_handle* h, const float* obs_dev, int32_t n, const float* eps_dev, int64_t step,
                            float* action_dev, float* clipped_dev, float* logp_dev);
int dsact_buffer_add_device(dsact_handle* h, int64_t n, const float* obs, const float* act, const float* rew, const float* obs2,
                            const uint8_t* terminated, const uint8_t* truncated, const float* logp, double reward_scale);

/* ---- Device-resident evaluation (training/hip_tensor_evaluator.py) -------------------------------------
 * The evaluation episodes of training/evaluator.py:34-84 for batched simulators whose observations, rewards and done flags live
 * on the GPU: N environments step in lockstep; a lockstep step costs launches only, and the loop waits in dsact_eval_poll alone.
 *   dsact_act_mode_device          training/evaluator.py:34-84's acting (logits = policy(obs), action = dist.mode(), lines
 *                                  47-51) for n environments with every operand on the device: obs[n*O] in, read in place;
 *                                  action[n*A] out. Bit for bit dsact_act_mode_batch's GPU route; the mode of a plain Gaussian
 *                                  is clamped to the action limits. Enqueued on the handle's stream behind every enqueued
 *                                  update: the LIVE weights, also under a behaviour hold (like dsact_act_mode_batch).
 *                                  ASYNCHRONOUS: no stream synchronisation, no host copy. All pointers must be device memory
 *                                  of the handle's GPU (DSACT_E_INVALID otherwise). Any n >= 1 (chunked inside the call); MLP
 *                                  policies with act_dim <= 32 (DSACT_E_INVALID for CNN policies without
 *                                  dsact_cnn_acting_enable).
 *   dsact_eval_begin               training/evaluator.py:34-84's bookkeeping (lines 40-46 and 77-81: the reward list and the
 *                                  episode loop) moved to the device: allocates (or grows) the state for n_envs rows and n_episodes
 *                                  episodes and initialises it in stream order -- row i plays episode i (none when
 *                                  i >= n_episodes), zeros elsewhere, remaining = n_episodes. Episode e runs on row e % n_envs,
 *                                  a row plays its episodes in index order. n_envs < 1 or n_episodes < 1: DSACT_E_INVALID.
 *   dsact_eval_commit              one lockstep step of training/evaluator.py:34-84 (lines 46-62 and 74: the reward is appended, the
 *                                  episode ends on done or a time-out, its return is the sum of its rewards) for every row
 *                                  in ONE launch: reward[n_envs] fp32, terminated / truncated [n_envs] one byte each (non-zero
 *                                  = set). ended[i] = terminated[i] | truncated[i] is written for every row (the mask of the
 *                                  environment's reset); a row with an episode adds the reward to its fp64 sum in step order
 *                                  and counts the step; at an end the episode's return and length are stored, the row goes
 *                                  on to episode e + n_envs (or to none) and `remaining` drops by one. ASYNCHRONOUS.
 *                                  DSACT_E_STATE before dsact_eval_begin; device pointers of the handle's GPU only.
 *   dsact_eval_poll                the number of episodes that have not ended, read behind everything enqueued so far: the
 *                                  counter is copied to pinned memory on the handle's stream and the call WAITS for it -- the
 *                                  only wait of the evaluation loop (training/evaluator.py:34-84 waits for every action).
 *   dsact_eval_read                waits, then copies returns[n_episodes] (fp64) and lengths[n_episodes] to the host: the
 *                                  episode returns training/evaluator.py:34-84 averages (lines 77-84). DSACT_E_STATE while an
 *                                  episode has not ended; n_episodes must be dsact_eval_begin's.
 * dsact_debug_get: "act_mode_dev_calls" (chunks launched by dsact_act_mode_device), "eval_commit_calls", "eval_polls";
 * "act_dev_syncs" stays 0 across dsact_act_mode_device and dsact_eval_commit too.
 *
 * UNDER STREAM CAPTURE (training/hip_tensor_evaluator.py with hip_graph_eval): a window of lockstep steps
 * is the same launch sequence every time -- the mode draws no noise, so no step counter is involved -- and may be captured from
 * the handle's stream into a graph. The rules are dsact_act_sample_device_counted's:
 *   dsact_act_mode_device          on an MLP handle is LEGAL WHILE THE HANDLE'S STREAM IS CAPTURING: it then allocates nothing
 *                                  (DSACT_E_STATE if no earlier call has made the batched forward's buffers: make one call outside
 *                                  the capture first), waits for nothing and leaves the hand-off check to the next entry point
 *                                  outside the capture. DSACT_E_STATE while profiling; DSACT_E_INVALID on a CNN handle (that route
 *                                  records an event per call), dsact_act_mode_device_u8 included -- unless the handle opted in
 *                                  with dsact_cnn_acting_capture (below).
 *   dsact_eval_commit              is legal under capture by the same rules (no hand-off check while capturing, DSACT_E_STATE
 *                                  while profiling). The captured node holds the ADDRESSES of the state dsact_eval_begin
 *                                  allocated, and dsact_eval_begin frees and reallocates that state when n_envs or n_episodes
 *                                  grows: dsact_debug_get "eval_state_gen" goes up by one on every (re)allocation, and a graph
 *                                  that holds a dsact_eval_commit node is valid only for the generation it was captured under
 *                                  (read it after dsact_eval_begin; replaying it under another one writes freed memory). N and
 *                                  E are baked as well: a replay serves the (n_envs, n_episodes) of the capture.
 *   dsact_eval_begin / dsact_eval_poll / dsact_eval_read   DSACT_E_STATE under capture: they allocate or wait.
 * "act_mode_dev_calls" and "eval_commit_calls" count HOST calls: they move when a graph is captured and not when it is replayed
 * (as "act_dev_calls" does for the counted sampling call). */
int dsact_act_mode_device(dsact_handle* h, const float* obs_dev, int32_t n, float* action_dev);

/* ---- Device-resident image environments ----------------------------------------------------------------
 * After dsact_cnn_acting_enable the device-resident forms above serve a CNN handle too (without it they answer as ever:
 * DSACT_E_INVALID "serves MLP policies" / "image rings" / "coded rings"):
 *   dsact_act_sample_device / dsact_act_mode_device   obs_dev holds n frames of O = C*H*W floats in the environment's (C, H, W)
 *       layout, 16-byte aligned, read in place; chunks of 64 frames run the CNN acting forward of dsact_act_sample_batch (frame
 *       ingest, conv stack, feature scatter, twin trunk, output launch) on the handle's stream with the live weights. With the
 *       same eps a row is bit for bit dsact_act_sample_batch's; drawn noise is the same function of (seed, step, row, d). No
 *       synchronisation, no host copy; every chunk counts in "act_dev_calls" / "act_mode_dev_calls". A held
 *       dsact_act_sample_batch that follows waits on its acting stream for an event recorded behind the last launch.
 *   dsact_buffer_add_device   fp32 image ring: the two image columns row by row (16-byte aligned sources), the narrow columns as
 *       for the MLP ring. Coded ring: the image columns are encoded as dsact_buffer_add encodes them; a value missing from the
 *       codebook makes the next dsact_buffer_add* / dsact_buffer_check fail, as there.
 * BYTE FRAMES (the _u8 forms; an enabled CNN handle WITH a coded ring, DSACT_E_STATE naming hip_obs_codebook without one): a frame
 * is C*H*W bytes in (C, H, W) layout, each a code into the ring's codebook -- the pixel is codebook[byte].
 *   dsact_act_sample_device_u8 / dsact_act_mode_device_u8   the calls above on byte frames: bit for bit their results on the
 *       decoded fp32 frames.
 *   dsact_buffer_add_device_u8   obs / obs2 are byte frames; they go to the code columns as they are (no search). A byte >=
 *       the codebook's size is a miss, recorded and reported like the encoder's (the byte as the value, its ring row). */
int dsact_act_sample_device_u8(dsact_handle* h, const uint8_t* frames_dev, int32_t n, const float* eps_dev, int64_t step,
                               float* action_dev, float* clipped_dev, float* logp_dev);
int dsact_act_mode_device_u8(dsact_handle* h, const uint8_t* frames_dev, int32_t n, float* action_dev);
int dsact_buffer_add_device_u8(dsact_handle* h, int64_t n, const uint8_t* obs, const float* act, const float* rew, const uint8_t* obs2,
                               const uint8_t* terminated, const uint8_t* truncated, const float* logp, double reward_scale);

/* ---- A sample() as one captured graph (training/hip_tensor_sampler.py with hip_graph_sample) ------------
 * The device-resident sampler's lockstep steps (training/off_sampler.py:46-84 for N environments) are about twenty launches
 * each, issued one at a time; captured into a graph they replay with one host call. A graph bakes every kernel argument, so the
 * acting step that keys the Philox draws (streams 5 and 6 above) comes from ONE 8-byte word in device memory the handle owns:
 *   dsact_act_counter_set(h, step)  writes the word in stream order (a one-lane launch that takes the value as its argument).
 *                                  The first call allocates the word. DSACT_E_STATE under stream capture: the value would be
 *                                  baked into the graph.
 *   dsact_act_counter_add(h, k)     word += k in stream order (a one-lane launch); k may be negative. Legal under stream capture:
 *                                  it is the node that closes a captured sample(), so every replay moves the counter on by the
 *                                  lockstep steps it made. DSACT_E_STATE before dsact_act_counter_set.
 *   dsact_act_counter_read(h, out)  WAITS for the handle's stream and copies the word to the host (tests, run_state()).
 *                                  DSACT_E_STATE before dsact_act_counter_set and under stream capture.
 *   dsact_act_sample_device_counted dsact_act_sample_device with eps == NULL and step = counter + step_offset (one 64-bit add in
 *                                  the kernel, carry included): the same checks, the same chunking (a row's noise does not
 *                                  depend on it), the same exploration-noise switch, bit for bit the same action / clipped /
 *                                  logp as dsact_act_sample_device(eps = NULL, step = counter + step_offset). The counter is read
 *                                  when the launch runs, behind every dsact_act_counter_* launch enqueued before it.
 *                                  DSACT_E_INVALID on CNN handles (served after dsact_cnn_acting_capture, below); DSACT_E_STATE before dsact_act_counter_set and without an
 *                                  acting seed. LEGAL WHILE THE HANDLE'S STREAM IS CAPTURING: it then allocates nothing
 *                                  (DSACT_E_STATE if no earlier call has made the batched forward's buffers: make one call outside
 *                                  the capture first), waits for nothing, and leaves the hand-off check to the next entry point
 *                                  outside the capture.
 *   dsact_step_rows_device          the row copies of one lockstep step (training/off_sampler.py:66-84: the step's next
 *                                  observation, reward and done flags kept for the batch) in ONE launch: obs2[n*row_floats],
 *                                  rew[n], terminated[n], truncated[n] (one byte each) are copied to the slots the caller names
 *                                  (row t*n of its [S, .] buffers) and ended[i] = terminated[i] | truncated[i] (0 or 1: the mask
 *                                  of the environment's reset) is written. Pure moves, 16 bytes per lane where row_floats % 4
 *                                  == 0 and source and slot are 16-byte aligned. ASYNCHRONOUS, legal under stream capture; device
 *                                  pointers of the handle's GPU only (DSACT_E_INVALID otherwise).
 * dsact_debug_get: "step_rows_calls" (dsact_step_rows_device launches); the counted call's chunks count in "act_dev_calls", and
 * "act_dev_syncs" stays 0 across all of the above but dsact_act_counter_read. */
int dsact_act_counter_set(dsact_handle* h, uint64_t step);
int dsact_act_counter_add(dsact_handle* h, int64_t k);
int dsact_act_counter_read(dsact_handle* h, uint64_t* out);
int dsact_act_sample_device_counted(dsact_handle* h, const float* obs_dev, int32_t n, int64_t step_offset, float* action_dev,
                                    float* clipped_dev, float* logp_dev);
int dsact_step_rows_device(dsact_handle* h, int32_t n, int32_t row_floats, const float* obs2_dev, const float* rew_dev,
                           const uint8_t* terminated_dev, const uint8_t* truncated_dev, float* obs2_slot, float* rew_slot,
                           uint8_t* terminated_slot, uint8_t* truncated_slot, uint8_t* ended_dev);
int dsact_eval_begin(dsact_handle* h, int32_t n_envs, int32_t n_episodes);
int dsact_eval_commit(dsact_handle* h, const float* reward_dev, const uint8_t* terminated_dev, const uint8_t* truncated_dev,
                      uint8_t* ended_dev);
int dsact_eval_poll(dsact_handle* h, int32_t* remaining);
int dsact_eval_read(dsact_handle* h, double* returns, int32_t* lengths, int32_t n_episodes);

/* ---- Image environments inside sample / eval graphs -----------------------------------------------------
 * The two capture sections above refuse a CNN handle: its device-resident acting calls record an event behind their last launch
 * (the fence a held dsact_act_sample_batch waits for), and a captured node cannot carry that event across replays.
 *   dsact_cnn_acting_capture(h, on)  the PER-HANDLE OPT-IN that lifts the refusal. Legal after dsact_cnn_acting_enable
 *                                  (DSACT_E_STATE otherwise) and outside a capture (DSACT_E_STATE). Default off: every call makes
 *                                  the runtime calls and gives the answers described above, both refusals and their messages
 *                                  included. STICKY: on = 0 after it was switched on is DSACT_E_STATE (on = 0 while off is a
 *                                  no-op) -- a graph captured under it may be replayed at any time. While on:
 *                                    - dsact_act_sample_device_counted, dsact_act_sample_device_counted_u8, dsact_act_mode_device
 *                                      and dsact_act_mode_device_u8 on this CNN handle are LEGAL WHILE THE HANDLE'S STREAM IS
 *                                      CAPTURING, by the MLP rules: DSACT_E_STATE "make one call outside the capture first"
 *                                      while the forward's lazily allocated buffers are missing, DSACT_E_STATE while profiling,
 *                                      no hand-off check under capture (left to the next entry point outside it).
 *                                    - NO device-resident CNN acting call records the event any more, captured or not.
 *                                    - a held host-row call (dsact_act_sample_batch / dsact_act_sample under
 *                                      dsact_behaviour_hold, on the acting stream) records the event ON THE HANDLE'S STREAM ITSELF
 *                                      and makes the acting stream wait for it. DSACT_E_STATE if that stream is capturing.
 *                                    - nothing records or waits for an event inside a capture and nothing forks: the graph
 *                                      is one linear chain on the handle's stream.
 *                                  WHY OPT-IN: the held call's fence moves from "behind the last device-resident acting call" to
 *                                  "behind EVERYTHING enqueued on the handle's stream at the held call" -- updates enqueued after
 *                                  that acting call included. The held call's results are the same bits (it reads the held
 *                                  copy of the weights); it may start later than it does without the switch.
 *   dsact_act_sample_device_counted  on an enabled CNN handle WITH the switch on: fp32 frames, 16-byte aligned, read in place; bit
 *                                  for bit dsact_act_sample_device(eps = NULL, step = counter + step_offset). Switch off:
 *                                  DSACT_E_INVALID as ever.
 *   dsact_act_sample_device_counted_u8  its byte-frame form (dsact_act_sample_device_u8's counted form): needs the switch and a
 *                                  coded ring -- DSACT_E_INVALID without the switch or off a CNN handle, DSACT_E_STATE naming
 *                                  hip_obs_codebook without a coded ring.
 *   dsact_step_frames_device        dsact_step_rows_device for IMAGE rows: a row is row_bytes bytes of any element type (a byte
 *                                  frame, an fp32 frame), split over several workgroups (k_step_rows moves a row with one
 *                                  wave). The same pure moves and ended[i] = (terminated[i] | truncated[i]) != 0. 16 bytes per
 *                                  lane where row_bytes % 16 == 0 and source and slot are 16-byte aligned, 4 bytes where
 *                                  everything is 4-aligned, bytes otherwise. ASYNCHRONOUS, legal under stream capture
 *                                  (DSACT_E_STATE while profiling); device pointers of the handle's GPU only. Any handle.
 * A captured CNN acting node holds the addresses of the path's buffers, the codebook and the limit arrays; none of them is ever
 * freed or reallocated before dsact_destroy (DESIGN.md section 24 has the lines), so there is no generation to watch.
 * dsact_debug_get: "cnn_act_capture" (the switch), "step_frames_calls" (dsact_step_frames_device launches). */
int dsact_cnn_acting_capture(dsact_handle* h, int32_t on);
int dsact_act_sample_device_counted_u8(dsact_handle* h, const uint8_t* frames_dev, int32_t n, int64_t step_offset, float* action_dev,
                                       float* clipped_dev, float* logp_dev);
int dsact_step_frames_device(dsact_handle* h, int32_t n, int64_t row_bytes, const void* obs2_dev, const float* rew_dev,
                             const uint8_t* terminated_dev, const uint8_t* truncated_dev, void* obs2_slot, float* rew_slot,
                             uint8_t* terminated_slot, uint8_t* truncated_slot, uint8_t* ended_dev);

/* ---- The evaluation trace: eval_save on the device (training/hip_tensor_evaluator.py) -------------------
 * The reference's Evaluator with eval_save keeps every evaluation episode's observations, actions and rewards and writes them
 * to save_folder/evaluator/iter{iteration}_ep{k}.npy. A device-resident evaluation never brings a row to the host, so the
 * handle keeps the lists of the FIRST n_saved episodes beside dsact_eval_begin's bookkeeping and hands them over at the end:
 *   tr_obs[n_saved][max_steps][obs_row_bytes] raw bytes, tr_act[n_saved][max_steps][act_dim] fp32, tr_rew[n_saved][max_steps]
 *   fp32, and one 64-bit `dropped` counter. The handle owns them; dsact_destroy frees them.
 *   dsact_eval_trace_begin         training/evaluator.py:40-42 (obs_list = [], action_list = [], reward_list = []) for episodes
 *                                  0 .. n_saved - 1 of the running evaluation (1 <= n_saved <= n_episodes), max_steps >= 1 slots
 *                                  each. Call it after dsact_eval_begin (DSACT_E_STATE before one). Allocates only on growth,
 *                                  after draining the handle's stream as dsact_eval_begin does; "eval_state_gen" goes up on
 *                                  every (re)allocation, so the guard of a graph with dsact_eval_commit nodes covers the trace's
 *                                  addresses too. `dropped` is zeroed in stream order by every call. obs_row_bytes must be the
 *                                  handle's observation row: 4 * obs_dim for MLP handles; C*H*W (byte frames) or 4*C*H*W (fp32
 *                                  frames) for image handles after dsact_cnn_acting_enable -- anything else DSACT_E_INVALID.
 *                                  DSACT_E_STATE under stream capture. n_saved and max_steps are baked into captured nodes.
 *   dsact_eval_trace_end           the trace goes inactive: later commits and records behave as without one (training/
 *                                  evaluator.py:62-73 is over: the dict has been handed out). The arrays are kept for the next
 *                                  begin. dsact_eval_begin is no substitute for this call, but every evaluation starts WITHOUT
 *                                  a trace: after dsact_eval_begin the trace is inactive until the next dsact_eval_trace_begin.
 *   dsact_eval_record              training/evaluator.py:53-54 (obs_list.append(obs); action_list.append(action)) for every row
 *                                  in ONE launch, issued BEFORE the environment steps: a row i that plays a saved episode
 *                                  (0 <= ep[i] < n_saved) copies its observation row (obs_row_bytes bytes of obs_dev, row-major)
 *                                  and its action row (act_dim floats of action_dev: the action the environment receives) into
 *                                  slot (ep[i], len[i]) when len[i] < max_steps; at len[i] >= max_steps it stores nothing and adds
 *                                  1 to `dropped`, once per (row, step). Every other row does nothing. A row is split over
 *                                  several workgroups like dsact_step_frames_device's; 16 bytes per lane where obs_row_bytes %
 *                                  16 == 0 and obs_dev is 16-byte aligned, 4 bytes where everything is 4-aligned, bytes
 *                                  otherwise; slot offsets are 64-bit. By dsact_eval_commit's rules: device pointers of the
 *                                  handle's GPU only (DSACT_E_INVALID), ASYNCHRONOUS, legal under stream capture (DSACT_E_STATE
 *                                  while profiling). DSACT_E_STATE without an active trace.
 *   dsact_eval_commit              with an active trace also stores the step's reward (training/evaluator.py:62:
 *                                  reward_list.append(reward)) at slot (e, len - 1), len the step count this commit reaches,
 *                                  when e < n_saved and len - 1 < max_steps. Everything else it does is unchanged.
 *   dsact_eval_trace_read          training/evaluator.py:62-73 (the dict of the three lists): WAITS, then copies rows =
 *                                  min(lengths[episode], max_steps) rows of one saved episode to obs_host (rows * obs_row_bytes
 *                                  bytes), act_host (rows * act_dim floats) and rew_host (rows floats). DSACT_E_STATE while an
 *                                  episode of the evaluation has not ended and without an active trace; DSACT_E_INVALID when
 *                                  episode is not 0 .. n_saved - 1 or capacity_rows < rows.
 * dsact_debug_get: "eval_record_calls" (dsact_eval_record launches, host calls as "eval_commit_calls"), "eval_trace_dropped" (the
 * counter AS IT STANDS, a blocking copy that does not wait for the handle's stream: read it after dsact_eval_read);
 * "act_dev_syncs" stays 0 across dsact_eval_record too. */
int dsact_eval_trace_begin(dsact_handle* h, int32_t n_saved, int32_t max_steps, int64_t obs_row_bytes);
int dsact_eval_trace_end(dsact_handle* h);
int dsact_eval_record(dsact_handle* h, const void* obs_dev, const float* action_dev);
int dsact_eval_trace_read(dsact_handle* h, int32_t episode, void* obs_host, float* act_host, float* rew_host, int32_t capacity_rows,
                          int32_t* rows);

/* ---- Episode statistics of the training environments (training/hip_tensor_sampler.py) ------------------
 * Returns and lengths of the episodes the device-resident sampler's N TRAINING environments play, kept on the device across
 * sample() calls: one launch per sample(), no wait unless the numbers are asked for. Per environment row i < n_envs the handle
 * keeps the episode in progress -- cur_ret[i] (fp64), cur_len[i] -- and the totals over the episodes of row i that ended since
 * the totals were last cleared: episodes[i], terminated[i] (episodes that ended with `terminated` set; both flags in one step
 * count here), ret_sum[i], ret_min[i] (+inf while none), ret_max[i] (-inf while none), len_sum[i], last_ret[i], last_len[i].
 *   dsact_track_begin              allocates the state for n_envs rows (or reallocates it when n_envs grows, after draining the
 *                                  handle's stream) and initialises ALL of it in stream order: new statistics.
 *                                  n_envs < 1: DSACT_E_INVALID.
 *   dsact_track_commit             n_steps lockstep steps in ONE launch: reward[n_steps * n_envs] fp32 (the environment's own
 *                                  reward, before any reward_scale), terminated / truncated [n_steps * n_envs] one byte each
 *                                  (non-zero = set), step-major (element t * n_envs + i is row i's step t: the sampler's
 *                                  buffers as they are). A row adds each reward to its fp64 running return in step order
 *                                  (dsact_eval_commit's rule) and counts the step; at terminated | truncated the episode is
 *                                  folded into the row's totals (min / max by strict comparison) and the running pair
 *                                  cleared. A row touches its own slots only -- no atomics, no reduction: every number is a
 *                                  pure function of the row's reward and flag sequence, however the steps are split into
 *                                  calls. ASYNCHRONOUS: no stream synchronisation, no host copy. DSACT_E_STATE before
 *                                  dsact_track_begin; n_steps < 1: DSACT_E_INVALID; device pointers of the handle's GPU only
 *                                  (host and pinned memory: DSACT_E_INVALID).
 *   dsact_track_read               copies the state to the host behind everything enqueued so far and WAITS for it -- the only
 *                                  wait of the feature -- into the caller's ten arrays of n_envs elements each. clear != 0:
 *                                  the totals' initialisation is then enqueued (counters and sums 0, ret_min = +inf, ret_max =
 *                                  -inf, last_* = 0); the episode in progress (cur_ret, cur_len) is NEVER cleared, so an
 *                                  episode that spans a read is counted whole. n_envs must be dsact_track_begin's
 *                                  (DSACT_E_INVALID); DSACT_E_STATE before dsact_track_begin.
 * dsact_destroy frees the state. dsact_debug_get: "track_commit_calls" (dsact_track_commit launches), "track_reads"
 * (dsact_track_read waits); "act_dev_syncs" stays 0 across dsact_track_commit too. */
int dsact_track_begin(dsact_handle* h, int32_t n_envs);
int dsact_track_commit(dsact_handle* h, const float* reward_dev, const uint8_t* terminated_dev, const uint8_t* truncated_dev,
                       int32_t n_steps);
int dsact_track_read(dsact_handle* h, int32_t n_envs, int64_t* episodes, int64_t* terminated, double* ret_sum, double* ret_min,
                     double* ret_max, int64_t* len_sum, double* last_ret, int32_t* last_len, double* cur_ret, int32_t* cur_len,
                     int32_t clear);

/* ---- The reference's environment wrappers on tensor environments (training/hip_tensor_env_wrappers.py) ---
 * utils/wrapping_env.py puts every environment behind gym's TimeLimit, ShapingRewardData ((r + shift) * scale) and
 * ScaleObservationData ((obs + shift) * scale). For a batched tensor environment the three are ONE launch behind step and ONE
 * behind reset. The handle keeps NO state: elapsed, the two parameter rows and the outputs are the caller's device arrays.
 *   dsact_env_wrap_step            n >= 1 rows. Each of the three parts is on or off:
 *                                    observation  row_floats > 0: obs2_out[i][k] = (obs2[i][k] + obs_shift[k]) * obs_scale[k], two
 *                                                 separately rounded fp32 operations; obs_shift_dev / obs_scale_dev hold one row of
 *                                                 row_floats floats. row_floats == 0: off.
 *                                    reward       reward_on != 0: rew_out[i] = (rew[i] + reward_shift) * reward_scale, likewise.
 *                                    time limit   max_episode_steps = M > 0: elapsed[i] = min(elapsed[i] + 1, M) (int32, saturating)
 *                                                 and truncated_out[i] = truncated[i] | (elapsed[i] >= M & ~terminated[i]), written
 *                                                 as 0 or 1 (flags are one byte each, non-zero = set) -- gym 0.23's
 *                                                 info["TimeLimit.truncated"] = not done, OR the environment's own truncation.
 *                                                 M == 0: off.
 *                                  obs2_out / rew_out / truncated_out must be NULL exactly when its part is off, an input of a part
 *                                  that is on must not be NULL, and at least one part must be on (DSACT_E_INVALID otherwise);
 *                                  inputs of a part that is off are ignored. An output may be its input (in place).
 *   dsact_env_wrap_reset           the observation part for EVERY row of obs_dev[n][row_floats] (row_floats == 0 and obs_out ==
 *                                  NULL: off) and, where elapsed_dev != NULL, elapsed[i] = 0 for the rows whose mask byte is
 *                                  non-zero (mask_dev == NULL: every row). At least one of the two must be on.
 * Both follow dsact_step_rows_device's rules: ASYNCHRONOUS on the handle's stream; legal under stream capture (no allocation, no
 * wait, the hand-off check left to the next entry point outside it; DSACT_E_STATE while profiling); device pointers of the
 * handle's GPU only (DSACT_E_INVALID otherwise). One wave per row and four rows per workgroup, rows above 1024 access units
 * split over up to 16 workgroups like dsact_step_frames_device's; 16 bytes per lane where row_floats % 4 == 0 and source, output
 * and both parameter rows are 16-byte aligned, 4 bytes otherwise. Any handle.
 * dsact_debug_get: "env_wrap_calls" (launches of either entry point). */
int dsact_env_wrap_step(dsact_handle* h, int32_t n, int32_t row_floats, const float* obs2_dev, const float* rew_dev,
                        const uint8_t* terminated_dev, const uint8_t* truncated_dev, const float* obs_shift_dev,
                        const float* obs_scale_dev, float reward_shift, float reward_scale, int32_t reward_on,
                        int32_t max_episode_steps, int32_t* elapsed_dev, float* obs2_out, float* rew_out, uint8_t* truncated_out);
int dsact_env_wrap_reset(dsact_handle* h, int32_t n, int32_t row_floats, const float* obs_dev, const uint8_t* mask_dev,
                         const float* obs_shift_dev, const float* obs_scale_dev, int32_t* elapsed_dev, float* obs_out);

/* ---- The reference's image pipeline on tensor environments (training/hip_tensor_frame_pipe.py) ----------
 * env_gym/gym_carracing_data.py feeds its networks the last img_stack gray frames and holds every action for action_repeat
 * simulator steps. For a batched tensor environment that is ONE launch behind each inner step and ONE behind a reset. The
 * handle keeps NO state: the stack, the scratch and the outputs are the caller's device arrays.
 * Row i owns a stack stack_dev[i][frame_stack][slot_elems]; a slot holds slot_elems output elements:
 *   gray == 0   the inner row raw_dev[i][slot_elems] in its own type, elem_size 1 or 4 bytes, moved as bits;
 *   gray == 1   raw_dev[i][3][slot_elems] (chw), gray == 2: raw_dev[i][slot_elems][3] (hwc); elements are bytes holding 0..255
 *               (elem_size 1) or fp32 (elem_size 4); a slot is slot_elems fp32 pixels
 *               float( ((R*0.299 + G*0.587) + B*0.114) / 128 - 1 ), computed in fp64 with every operation rounded on its own
 *               (gym_carracing_data.py:63-69).
 *   dsact_frame_pipe_step   launch j of action_repeat, issued behind inner step j (gym_carracing_data.py:34-51). A row is
 *                           alive until an inner step sets terminated | truncated for it. For a row alive at the start of j:
 *                           j == 0 shifts the stack by one slot and writes the newest slot from raw_dev, j > 0 overwrites the
 *                           newest slot; acc = rew (j == 0) or acc + rew, one rounded fp32 add; the step that ends the row
 *                           keeps its two flags and sets ended_at[i] = j (ended_at is -1 while alive; j == 0 writes it
 *                           outright, so the three scratch arrays acc_dev[n] / ended_at_dev[n] / flags_dev[n] need no
 *                           initialisation). At j == action_repeat - 1 every row copies its stack to obs2_out and
 *                           rew_out / terminated_out / truncated_out (0 or 1) are written. No pointer may be NULL.
 *   dsact_frame_pipe_reset  rows whose mask byte is non-zero (mask_dev == NULL: every row) fill all frame_stack slots from
 *                           raw_dev[i] (gym_carracing_data.py:23-32); every row then copies its stack to obs_out.
 * DSACT_E_INVALID with a message and no launch: n < 1, frame_stack < 1, slot_elems < 1, action_repeat < 1, j outside
 * [0, action_repeat), a NULL pointer other than mask_dev, gray outside {0, 1, 2}, elem_size outside {1, 4}, a pointer off the
 * handle's GPU. Both follow dsact_env_wrap_step's rules: ASYNCHRONOUS on the handle's stream; legal under stream capture (no
 * allocation, no wait; DSACT_E_STATE while profiling). One wave per row and four rows per workgroup, rows above 1024 access
 * units split over up to 16 workgroups; a unit is 16 bytes of a slot where the element counts and the pointers' alignment
 * allow, one element otherwise. Any handle.
 * dsact_debug_get: "frame_pipe_calls" (launches of either entry point). */
int dsact_frame_pipe_step(dsact_handle* h, int32_t n, int64_t slot_elems, int32_t frame_stack, int32_t action_repeat, int32_t j,
                          int32_t gray, int32_t elem_size, const void* raw_dev, const float* rew_dev, const uint8_t* terminated_dev,
                          const uint8_t* truncated_dev, void* stack_dev, float* acc_dev, int32_t* ended_at_dev, uint8_t* flags_dev,
                          void* obs2_out, float* rew_out, uint8_t* terminated_out, uint8_t* truncated_out);
int dsact_frame_pipe_reset(dsact_handle* h, int32_t n, int64_t slot_elems, int32_t frame_stack, int32_t gray, int32_t elem_size,
                           const void* raw_dev, const uint8_t* mask_dev, void* stack_dev, void* obs_out);

#ifdef __cplusplus
}
#endif
#endif /* DSACT_H */
