// dsact_act_batch.h -- the vectorised sampler's acting forward: policy(obs) + the action distribution's sample() for n
// observation rows per call (training/off_sampler.py:46-56 over N environments, networks/mlp.py:79-100,
// utils/act_distribution_cls.py:32-42 and :82-115), reading the live policy weights from the parameter arena on the
// handle's stream.
//
// Launch shape: one launch per layer, each a grid of (feature slice x row tile) workgroups; the output layer's launch also
// draws the action and its log-probability. Why not the one-launch hand-off of k_act_mlp (dsact_act.h): a dependent kernel
// boundary on the same stream costs ~1.5 us on the MI355X, the same order as one in-launch hop, and
// with n rows every layer hands over n x width values instead of one row -- a hop's price grows with the bytes a consumer
// reads, a boundary's does not. Why not one workgroup per row block: the whole 3 x 256 Humanoid policy (0.94 MB) through
// one CU took ~40 us (dsact_act.h); here a hidden layer's weights are split into 32-feature slices (a 256-wide layer: 8
// workgroups per row tile, each streaming 32 KB), so even n <= 32 spreads a layer over several CUs.
//
// Arithmetic: plain fp32 FMAs on the VALU, staged through LDS in 128-wide K chunks (the next chunk's loads are in flight
// while the current one is multiplied). At n <= 1024 and widths <= 1024 a layer is <= 1 GFMA: MFMA throughput buys nothing
// measurable against the launch boundaries, and a VALU dot product fixes the order of every sum: output (r, f) is
// fmaf(W[f][k], x[r][k], acc) for k = 0 .. K-1 in order, then + bias -- the same instructions whatever n is and wherever row
// r sits in its tile (rows never share a sum, padding only ever adds exact zeros after the last term). A row's action
// and log-probability are therefore bitwise independent of the batch around it. The sampling epilogue is tanh_gauss_fwd of
// dsact_math.h (the closed form k_act_mlp and the host acting path use; half range 0 selects the plain Gaussian), and the
// log-probability is summed over the action dimensions in order, as dsact_host_act.h's head() does.
//
// The evaluator's deterministic acting (training/evaluator.py:50-72 over N environments, dist.mode()) is the same output
// launch with kMode = true: the K loop, its sums and the output activation are the sampling form's instruction for
// instruction (a row's mean is bitwise the sampling kernel's), only the epilogue differs -- act_mode of dsact_math.h writes
// the action, no eps is read and no log-probability is reduced.
//
// The device-resident sampler's acting (training/hip_tensor_sampler.py, dsact_act_sample_device; training/off_sampler.py:46-65
// over N environments of a batched simulator) is the sampling form with kDev = true: the same K loop, sums, output activation
// and tanh_gauss_fwd (a row's action and log-probability are bitwise the sampling kernel's for the same eps), but
//   * eps comes from a device array, or -- eps == nullptr -- is drawn here: normal4 / philox4x32 (dsact_kernels.h) with stream id
//     kActStream = 5 (1 .. 3: the update noise, 4: the index draw), counter (row * ceil(A/4) + d/4, step low, step high, 5), key =
//     the acting seed, element d % 4 of the four normals. `row` is the environment's row in the whole call (row0 + the row in
//     this launch), `step` the caller's 64-bit acting-step counter: the noise of environment i at step t is a pure function of
//     (seed, t, i, d) -- independent of N and of the chunking at kActBatchCap;
//   * action[n][A], logp[n] and clipped[n][A] = min(max(action, lo), hi) (the value the environment receives,
//     off_sampler.py:62-65) are written to DEVICE memory the caller owns; nothing is mapped to the host.
//
// The device-resident evaluator's acting (training/hip_tensor_evaluator.py, dsact_act_mode_device; training/evaluator.py:50-72
// over N environments of a batched simulator) is the mode form with kDev = true -- k_act_batch_out<true, true>: the K loop, sums,
// output activation and act_mode of <true, false> (a row's action is bitwise dsact_act_mode_batch's GPU route), launched on obs
// the hidden layers read IN PLACE from the caller's device array (no staging copy) with action[n][A] in the caller's DEVICE
// memory. No eps is read, no logp, clipped, seed, step or row0: act_mode already clamps the plain Gaussian to the limits.
//
// CNN policies (dsact_cnn_acting_enable; training/off_sampler.py:46-56 on image observations,
// networks/cnn.py:151-240): k_act_frames below turns a chunk of <= kActFrameCap frames into the pixel-major rows k_conv_fwd
// reads, the conv stack and k_feat_scatter (dsact_conv.h) make the feature rows, and the launches above run the twin trunk
// (ActBatchHidden::half) and the sample on them. The device-resident forms run the same chunks with kDev = true on frames read in
// place; k_act_frames_u8 is the ingest for byte frames, codes into the coded ring's table.
//
// Exploration noise (dsact_set_explore_noise; training/off_sampler.py:58-65, utils/explore_noise.py:17-23):
// k_act_batch_out<false, true, true> is the device-resident sampling form with `action + N(mean, std)` in its epilogue. The
// normal is the acting draw's generator on stream id kExploreStream = 6: counter ((row0 + r) * ceil(A/4) + (shared ? 0 : d/4),
// step low, step high, 6), key = the acting seed, element shared ? 0 : d % 4 -- never a counter block of eps. Then
//   noise = __fmaf_rn(std[k], z, mean[k]) (k = shared ? 0 : d);  a = g.a + noise;  action = a;  clipped = min(max(a, lo), hi)
// with g = tanh_gauss_fwd(...) as ever: logp is that of the un-noised sample, and the ring gets the un-clipped noised action.
//
// The counted forms (dsact_act_sample_device_counted): k_act_batch_out<false, true, kExplore, true> is the
// device-resident sampling form whose acting step is `*step_ptr + step` -- the handle's 8-byte counter in device memory plus the
// launch's offset, one 64-bit add -- instead of the argument alone. A captured graph bakes its kernel arguments; the counter is
// read when the launch RUNS, so every replay draws the noise of its own steps. Both Philox draws (streams 5 and 6) use the sum;
// everything else is the uncounted form's instruction for instruction (same bits for the same effective step). The word is read
// with one ordinary load per lane of the same address (a wave: one request), behind the kernel boundary that orders it with the
// k_counter_add / k_counter_set launch that wrote it.
#pragma once
#include "dsact_kernels.h"
#include "dsact_conv.h"   // fast_div

namespace dsact {

constexpr int kActBatchCap = 1024;   // rows per launch; dsact_act_sample_batch chunks above it
constexpr int kAbKC = 128;           // K chunk of the hidden layers staged in LDS (a layer is a chain of chunk round trips)

// one hidden layer: Y[r][f] = act(sum_k W[f][k] X[r][xoff + k] + b[f]) for r < n, f < N. half > 0: a twin-trunk layer
// (policy_std_type "mlp_separated"): features >= half are the second trunk's and read inputs [K, 2K) (xoff = K)
struct ActBatchHidden {
  const float* X; int ldx;
  const float* W; const float* b;
  int K, N, half;
  float* Y; int ldy;
  int n, act;
};

// the output layer (2A <= 64 features) + the sample: action[r][d], logp[r]; with kMode the mode: action[r][d] only
struct ActBatchOut {
  const float* X; int ldx;
  const float* W; const float* b;
  int K, A, n;
  int out_act, out_n;                  // policy_output_activation and the outputs it applies to (2A, or A: mean half only)
  const float* eps;                    // [n][A] standard-normal draws
  const float* scale; const float* center;   // action half range / centre (0 / 0: GaussDistribution)
  const float* lo; const float* hi;          // action limits (kMode only: GaussDistribution.mode() clamps to them)
  float lo_ls, hi_ls;
  float* action; float* logp;          // [n][A], [n] (kMode: logp unused)
  // kDev only (appended: the other forms' argument offsets are what they were)
  float* clipped;                      // [n][A] the action clamped to [lo, hi]
  unsigned long long seed;             // the acting seed (eps == nullptr: the draw is made here)
  long long step;                      // the acting-step counter
  int row0;                            // the first row of this launch in the whole call (the chunk offset)
  // kExplore only (appended likewise): the exploration noise of dsact_set_explore_noise, device arrays the handle owns
  const float* ex_mean; const float* ex_std;   // [1] (ex_shared) or [A]
  int ex_shared;                       // one normal per row, added to every action dimension
  // kCounted only (appended likewise): the handle's acting-step counter in device memory (dsact_act_counter_set)
  const unsigned long long* step_ptr;  // the draws are keyed by *step_ptr + step (64 bits, carry included)
};
constexpr uint32_t kActStream = 5u;
constexpr uint32_t kExploreStream = 6u;

// frame ingest of the CNN acting forward: n frames as the environment delivers them, src[r][c][pix] (C, H, W), into the
// pixel-major rows of the conv kernels, dst[r][pix][c]. A pure permutation: no index table, no replay columns, no step
// bookkeeping, noise or weight repack (k_gather_img carries those for the update) -- it may run on any stream
constexpr int kActFrameCap = 64;     // frames per chunk of the CNN acting forward (the rows of the stand-alone forward)
struct ActFramesArgs {
  const float* src; float* dst;
  int n, C, HW;
  int chunks;                          // workgroups per frame
};
// the same ingest for BYTE frames (dsact_act_sample_device_u8 / dsact_act_mode_device_u8): src[r][c][pix] is
// one code per element into the coded ring's table, the pixel is book[code] -- the value k_gather_img_coded hands the update for
// that code, so acting and learning see the same bits
struct ActFramesU8Args {
  const uint8_t* src; float* dst;
  const float* book; int n_codes;
  int n, C, HW;
  int chunks;                          // workgroups per frame
  int grp;                             // C == 3 | 4, HW % 4 == 0 and a 4-byte aligned src: the 4-pixel group form
};

#ifdef DSACT_ACT_BATCH_DEFINE   // the kernels themselves: csrc/dsact_tu_act_batch.hip; other units see the declarations
// 32 rows x 32 features per workgroup; thread (tr, tf) = (tid / 16, tid % 16) owns rows tr, tr + 16 and features tf, tf + 16.
// grid: x = feature slices (per trunk), y = row tiles
__global__ void __launch_bounds__(256) k_act_batch_hidden(ActBatchHidden a) {
  __shared__ float xs[32][kAbKC + 1];
  __shared__ float ws[32][kAbKC + 1];
  const int tid = threadIdx.x, tf = tid & 15, tr = tid >> 4;
  const int seg_n = a.half > 0 ? a.half : a.N;
  const int tps = (seg_n + 31) / 32;
  const int seg = (int)blockIdx.x / tps;
  const int f0 = seg * seg_n + ((int)blockIdx.x % tps) * 32;
  const int f_end = min(f0 + 32, (seg + 1) * seg_n);
  const int r0 = (int)blockIdx.y * 32;
  const float* X = a.X + (seg ? a.K : 0);
  // staging: element e = tid + 256 q of a chunk is row e / kAbKC, column e % kAbKC (a wave: one 256-byte row segment per load)
  constexpr int QH = 32 * kAbKC / 256;
  float xr[QH], wr[QH];
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < QH; ++q) {
      const int e = tid + 256 * q, rr = e / kAbKC, k = k0 + e % kAbKC;
      xr[q] = (r0 + rr < a.n && k < a.K) ? X[(size_t)(r0 + rr) * a.ldx + k] : 0.f;
      wr[q] = (f0 + rr < f_end && k < a.K) ? a.W[(size_t)(f0 + rr) * a.K + k] : 0.f;
    }
  };
  load(0);
  float c00 = 0.f, c01 = 0.f, c10 = 0.f, c11 = 0.f;   // c<row i><feature j>
  for (int k0 = 0; k0 < a.K; k0 += kAbKC) {
    __syncthreads();   // the previous chunk's reads are done
#pragma unroll
    for (int q = 0; q < QH; ++q) {
      const int e = tid + 256 * q;
      xs[e / kAbKC][e % kAbKC] = xr[q];
      ws[e / kAbKC][e % kAbKC] = wr[q];
    }
    __syncthreads();
    if (k0 + kAbKC < a.K) load(k0 + kAbKC);   // (block-uniform) the next chunk's loads fly while this one is multiplied
#pragma unroll 16
    for (int kk = 0; kk < kAbKC; ++kk) {
      const float x0 = xs[tr][kk], x1 = xs[tr + 16][kk], w0 = ws[tf][kk], w1 = ws[tf + 16][kk];
      c00 = fmaf(w0, x0, c00); c01 = fmaf(w1, x0, c01);
      c10 = fmaf(w0, x1, c10); c11 = fmaf(w1, x1, c11);
    }
  }
  const float c[2][2] = {{c00, c01}, {c10, c11}};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = r0 + tr + 16 * i;
    if (r >= a.n) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int f = f0 + tf + 16 * j;
      if (f >= f_end) continue;
      float hv, gd;
      act_fwd_grad(a.act, c[i][j] + a.b[f], hv, gd);
      a.Y[(size_t)r * a.ldy + f] = hv;
    }
  }
}

// 8 rows x 64 outputs (mean | raw log-std, 2A <= 64) per workgroup; thread (tr, tf) = (tid / 32, tid % 32) owns row tr and
// outputs tf, tf + 32. grid: x = row tiles. kMode: the mode instead of the sample (eps and logp are not touched). kDev: the
// device-resident form (see the header comment; with kMode it is the mode epilogue on the caller's device arrays). kExplore
// (<false, true, true> only): exploration noise on the sampled action, before the clip. kCounted (<false, true, ., true> only): the
// acting step is *step_ptr + step
template <bool kMode, bool kDev, bool kExplore = false, bool kCounted = false>
__global__ void __launch_bounds__(256) k_act_batch_out(ActBatchOut a) {
  constexpr int KC = 64;   // (the 64-row weight tile at 128 columns runs out of scalar registers)
  __shared__ float xs[8][KC + 1];
  __shared__ float ws[64][KC + 1];
  __shared__ float raw[8][65];
  __shared__ float lps[8][33];
  const int tid = threadIdx.x, tf = tid & 31, tr = tid >> 5;
  const int r0 = (int)blockIdx.x * 8, N = 2 * a.A;
  constexpr int QX = 8 * KC / 256, QW = 64 * KC / 256;   // staging as in k_act_batch_hidden
  float xr[QX], wr[QW];
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < QX; ++q) {
      const int e = tid + 256 * q, rr = e / KC, k = k0 + e % KC;
      xr[q] = (r0 + rr < a.n && k < a.K) ? a.X[(size_t)(r0 + rr) * a.ldx + k] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < QW; ++q) {
      const int e = tid + 256 * q, rr = e / KC, k = k0 + e % KC;
      wr[q] = (rr < N && k < a.K) ? a.W[(size_t)rr * a.K + k] : 0.f;
    }
  };
  load(0);
  float c0 = 0.f, c1 = 0.f;
  for (int k0 = 0; k0 < a.K; k0 += KC) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < QX; ++q) { const int e = tid + 256 * q; xs[e / KC][e % KC] = xr[q]; }
#pragma unroll
    for (int q = 0; q < QW; ++q) { const int e = tid + 256 * q; ws[e / KC][e % KC] = wr[q]; }
    __syncthreads();
    if (k0 + KC < a.K) load(k0 + KC);
#pragma unroll 16
    for (int kk = 0; kk < KC; ++kk) {
      const float x = xs[tr][kk];
      c0 = fmaf(ws[tf][kk], x, c0);
      c1 = fmaf(ws[tf + 32][kk], x, c1);
    }
  }
  // (mean | raw log-std) of this row after policy_output_activation (networks/mlp.py:15-20)
  const float c[2] = {c0, c1};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = tf + 32 * j;
    if (f < N) {
      float z = c[j] + a.b[f];
      if (a.out_act && f < a.out_n) z = out_act_fwd(a.out_act, z);
      raw[tr][f] = z;
    }
  }
  __syncthreads();
  const int r = r0 + tr, d = tf;
  if constexpr (kMode) {   // dist.mode(), one (row, action dimension) per thread
    if (r < a.n && d < a.A) a.action[(size_t)r * a.A + d] = act_mode(raw[tr][d], a.scale[d], a.center[d], a.lo[d], a.hi[d]);
    return;
  }
  // the sample, one (row, action dimension) per thread: tanh_gauss_fwd term for term
  if constexpr (kDev) {
    // eps from the caller's device array or drawn here; then tanh_gauss_fwd as below, plus the clipped copy
    if (r < a.n && d < a.A) {
      long long step = a.step;
      if constexpr (kCounted) step = (long long)(*a.step_ptr + (unsigned long long)a.step);
      float e;
      if (a.eps) {
        e = a.eps[(size_t)r * a.A + d];
      } else {
        float z[4];
        normal4(a.seed, step, kActStream, (uint32_t)(a.row0 + r) * (uint32_t)((a.A + 3) >> 2) + (uint32_t)(d >> 2), z);
        const int q = d & 3;
        e = q == 0 ? z[0] : q == 1 ? z[1] : q == 2 ? z[2] : z[3];
      }
      const TanhGaussFwd g = tanh_gauss_fwd(raw[tr][d], raw[tr][a.A + d], e, a.scale[d], a.center[d], a.lo_ls, a.hi_ls);
      float act = g.a;
      if constexpr (kExplore) {
        float z[4];
        normal4(a.seed, step, kExploreStream,
                (uint32_t)(a.row0 + r) * (uint32_t)((a.A + 3) >> 2) + (a.ex_shared ? 0u : (uint32_t)(d >> 2)), z);
        const int q = a.ex_shared ? 0 : d & 3, k = a.ex_shared ? 0 : d;
        const float zq = q == 0 ? z[0] : q == 1 ? z[1] : q == 2 ? z[2] : z[3];
        act = g.a + __fmaf_rn(a.ex_std[k], zq, a.ex_mean[k]);
      }
      a.action[(size_t)r * a.A + d] = act;
      a.clipped[(size_t)r * a.A + d] = fminf(fmaxf(act, a.lo[d]), a.hi[d]);
      lps[tr][d] = g.lp;
    }
  } else {
  if (r < a.n && d < a.A) {
    const TanhGaussFwd g = tanh_gauss_fwd(raw[tr][d], raw[tr][a.A + d], a.eps[(size_t)r * a.A + d], a.scale[d], a.center[d],
                                          a.lo_ls, a.hi_ls);
    a.action[(size_t)r * a.A + d] = g.a;
    lps[tr][d] = g.lp;
  }
  }
  __syncthreads();
  // Independent(..., 1): the log-probability summed over the action dimensions, in order
  if (tid < 8 && r0 + tid < a.n) {
    float lp = 0.0f;
    for (int q = 0; q < a.A; ++q) lp += lps[tid][q];
    a.logp[r0 + tid] = lp;
  }
}
// grid: x = frame * chunks + chunk. C == 3 with HW % 4 == 0: a lane takes 4 consecutive pixels -- one 16-byte load per plane
// (a wave reads 1 KB of each plane back to back), the 3 x 4 block transposed in registers, three 16-byte stores (a wave writes
// 3 KB back to back): k_gather_img's RGB path for one image. Otherwise a lane per output quad, its 4 floats from <= 4 planes
// (fast_div by C; C * HW % 4 == 0 is checked when the handle is created)
__global__ void __launch_bounds__(256) k_act_frames(ActFramesArgs a) {
  const int r = (int)blockIdx.x / a.chunks, ck = (int)blockIdx.x - r * a.chunks;
  if (r >= a.n) return;
  const size_t O = (size_t)a.C * a.HW;
  const float* so = a.src + (size_t)r * O;
  float* d0 = a.dst + (size_t)r * O;
  if (a.C == 3 && (a.HW & 3) == 0) {
    const int nq = a.HW >> 2;
    for (int q = ck * 256 + (int)threadIdx.x; q < nq; q += a.chunks * 256) {
      f32x4 p[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = *(const f32x4*)(so + (size_t)c * a.HW + 4 * q);
#pragma unroll
      for (int j = 0; j < 3; ++j) {     // output quad j holds elements 4j .. 4j+3 of (pixel e, channel c) = e*3 + c
        f32x4 v;
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const int o = 4 * j + e4;
          v[e4] = p[o % 3][o / 3];
        }
        *(f32x4*)(d0 + (size_t)q * 12 + 4 * j) = v;
      }
    }
    return;
  }
  const int n4 = (int)(O >> 2);
  const float inv_c = 1.0f / (float)a.C;
  for (int q = ck * 256 + (int)threadIdx.x; q < n4; q += a.chunks * 256) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = q * 4 + e;
      const int pix = fast_div(o, a.C, inv_c), c = o - pix * a.C;
      v[e] = so[(size_t)c * a.HW + pix];
    }
    *(f32x4*)(d0 + (size_t)q * 4) = v;
  }
}
// k_act_frames for byte frames. The table sits in LDS, padded with 0 beyond n_codes (as k_ring_write_img_coded pads it).
// grp (CT = 3 | 4 channels): a lane takes a 4-pixel group -- ONE 4-byte load of codes per plane (a wave reads 256 bytes of each
// plane back to back), CT x 4 table reads, CT 16-byte stores (a wave writes CT KB back to back): the decode and store pattern
// of k_gather_img_coded<CT>. 16 pixels per lane from one 16-byte load were considered and not taken: the launch moves 4 output
// bytes per input byte, so a lane of the 4-pixel form already issues CT dwordx4 stores and 4 CT LDS reads per dword load -- the
// loads are 1 of 1 + 5 CT vector-memory / LDS instructions, and 4x the waves hide the table reads (the reasoning
// k_ring_write_img_coded records for its search). Otherwise a lane per output quad, its 4 codes read as bytes
// from <= 4 planes (fast_div by C). Vector loads and stores only; every access is inside frame r < n
template <int CT>
__device__ __forceinline__ void act_frames_u8_groups(const ActFramesU8Args& a, const float* tab, const uint8_t* so, float* d0, int ck) {
  const int nq = a.HW >> 2;
  for (int q = ck * 256 + (int)threadIdx.x; q < nq; q += a.chunks * 256) {
    uint32_t w[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) w[c] = *(const uint32_t*)(so + (size_t)c * a.HW + 4 * q);
#pragma unroll
    for (int j = 0; j < CT; ++j) {     // output quad j holds elements 4j .. 4j+3 of (pixel e, channel c) = e*CT + c
      f32x4 v;
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int o = 4 * j + e4;
        v[e4] = tab[(w[o % CT] >> (8 * (o / CT))) & 255u];
      }
      *(f32x4*)(d0 + (size_t)q * (4 * CT) + 4 * j) = v;
    }
  }
}
__global__ void __launch_bounds__(256) k_act_frames_u8(ActFramesU8Args a) {
  __shared__ float tab[256];
  tab[threadIdx.x] = (int)threadIdx.x < a.n_codes ? a.book[threadIdx.x] : 0.f;
  __syncthreads();
  const int r = (int)blockIdx.x / a.chunks, ck = (int)blockIdx.x - r * a.chunks;
  if (r >= a.n) return;
  const size_t O = (size_t)a.C * a.HW;
  const uint8_t* so = a.src + (size_t)r * O;
  float* d0 = a.dst + (size_t)r * O;
  if (a.grp && a.C == 3) { act_frames_u8_groups<3>(a, tab, so, d0, ck); return; }
  if (a.grp && a.C == 4) { act_frames_u8_groups<4>(a, tab, so, d0, ck); return; }
  const int n4 = (int)(O >> 2);
  const float inv_c = 1.0f / (float)a.C;
  for (int q = ck * 256 + (int)threadIdx.x; q < n4; q += a.chunks * 256) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = q * 4 + e;
      const int pix = fast_div(o, a.C, inv_c), c = o - pix * a.C;
      v[e] = tab[so[(size_t)c * a.HW + pix]];
    }
    *(f32x4*)(d0 + (size_t)q * 4) = v;
  }
}
template __global__ void k_act_batch_out<false, false>(ActBatchOut);
template __global__ void k_act_batch_out<true, false>(ActBatchOut);
template __global__ void k_act_batch_out<false, true>(ActBatchOut);
template __global__ void k_act_batch_out<true, true>(ActBatchOut);
template __global__ void k_act_batch_out<false, true, true>(ActBatchOut);
template __global__ void k_act_batch_out<false, true, false, true>(ActBatchOut);
template __global__ void k_act_batch_out<false, true, true, true>(ActBatchOut);
#else
__global__ void k_act_batch_hidden(ActBatchHidden a);
__global__ void k_act_frames(ActFramesArgs a);
__global__ void k_act_frames_u8(ActFramesU8Args a);
template <bool kMode, bool kDev, bool kExplore = false, bool kCounted = false>
__global__ void k_act_batch_out(ActBatchOut a);
extern template __global__ void k_act_batch_out<false, false>(ActBatchOut);
extern template __global__ void k_act_batch_out<true, false>(ActBatchOut);
extern template __global__ void k_act_batch_out<false, true>(ActBatchOut);
extern template __global__ void k_act_batch_out<true, true>(ActBatchOut);
extern template __global__ void k_act_batch_out<false, true, true>(ActBatchOut);
extern template __global__ void k_act_batch_out<false, true, false, true>(ActBatchOut);
extern template __global__ void k_act_batch_out<false, true, true, true>(ActBatchOut);
#endif

}  // namespace dsact
