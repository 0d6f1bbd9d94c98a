// Row-slice chain on v_mfma_f32_4x4x1_16b_f32: 16 blocks of (4 rows x 4 outputs, K = 1) per instruction, 8 cycles.
// lane n <-> output feature (64 per wave), the 4 accumulator registers <-> 4 batch rows, so an R = 8 row slice is two
// accumulator groups. Packed weights: [wave tile of 64 outputs][k/4][lane][4 k].
//
// The product step is the one of gemm44_seg (csrc/dsact_chain.h): trips of kPD = 16 steps, each step = 4 * RG MFMAs on two
// accumulators per row group, its weight slot refilled after its last use from the stream's next kPD steps (which run on
// into the next layer's weights: the stream never drains between layers), the LDS operand fetched D steps ahead into a
// register ring. Variants, to find out what in the step costs its cycles beyond 32 * RG of MFMA:
//   D     operand look-ahead in steps (the ring; reads that would cross the end of the layer wrap to the trip's own first steps)
//   SLOT  RG == 1 only: the operand read is issued BETWEEN the two MFMA pairs of a step (fills the accumulator hazard slot
//         that is an s_nop otherwise) instead of ahead of them
//   SADR  the stream base is held in SGPRs (readfirstlane) + one 32-bit lane offset; without it the wave's tile pointer is
//         not provably uniform and every refill carries a 64-bit VGPR address (the upper bound of what scalar addressing buys:
//         the library's kernels had that form on 12 of a trip's 16 refills)
// usage: slice_gemm44 [n_chains] [slices] [rounds]      per-layer time = (t(L = 9) - t(L = 3)) / 6, min / median / max over rounds
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <algorithm>
#include <vector>
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int W = 256, LDX = W + 8, kPD = 16, KS = W / 4;
__device__ __forceinline__ f32x4 gload4(const float* p) { return *(const __attribute__((address_space(1))) f32x4*)p; }
// a wave-uniform pointer pinned in an SGPR pair (the constraint makes the compiler read the first lane where it cannot prove
// uniformity) and opaque to instruction selection, which otherwise folds base + 4 KB * k into 64-bit VGPR addresses
__device__ __forceinline__ const float* sgpr_ptr(const float* p) { asm("" : "+s"(p)); return p; }

struct WStr { f32x4 b[kPD]; };

// one layer: KS steps of `cur` (this wave's tile), refills from `cur`, then from `nxt` (has_nxt) -- gemm44_seg's shape
template <int RG, int D, bool SLOT, bool SADR>
__device__ __forceinline__ void seg(WStr& ws, const float* cur, const float* nxt, bool has_nxt, const float* xs, int xi, int lane4,
                                    f32x4 (&acc)[RG][2]) {
  static_assert(D >= 1 && D <= 7 && (!SLOT || RG == 1), "ring of 8 named slots, D + 1 of them live");
  f32x4 a[8][RG];
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int g = 0; g < RG; ++g) a[j][g] = *(const f32x4*)(xs + xi + 4 * g * LDX + 4 * j);
  for (int s0 = 0; s0 < KS; s0 += kPD) {
    const bool last = !(s0 + kPD < KS);
    const float* src = !last ? cur + (size_t)(s0 + kPD) * 256 : (has_nxt ? nxt : cur);
    const float* sb[kPD / 4];   // one base per 4 KB: the 13-bit immediate of a global load reaches the 4 steps behind each
#pragma unroll
    for (int k = 0; k < kPD / 4; ++k) sb[k] = SADR ? sgpr_ptr(src + (size_t)k * 1024) : src + (size_t)k * 1024;   // (SADR: src is provably uniform here)
    const int xt = xi + 4 * s0, xw = last ? xt - 4 * kPD : xt;   // reads past the layer's end wrap to this trip's first steps
#pragma unroll
    for (int u = 0; u < kPD; ++u) {
      constexpr int DR = D;   // a slot-placed read is issued half a step later: D - 1/2 steps ahead of its use
      if (!SLOT) {
#pragma unroll
        for (int g = 0; g < RG; ++g) a[(u + DR) & 7][g] = *(const f32x4*)(xs + (u + DR < kPD ? xt : xw) + 4 * g * LDX + 4 * (u + DR));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int g = 0; g < RG; ++g)
          acc[g][e & 1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[u & 7][g][e], ws.b[u][e], acc[g][e & 1], 0, 0, 0);
        if (e == 1) {
          __builtin_amdgcn_sched_barrier(0);
          if (SLOT) {
            a[(u + DR) & 7][0] = *(const f32x4*)(xs + (u + DR < kPD ? xt : xw) + 4 * (u + DR));
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      ws.b[u] = gload4(sb[u >> 2] + (size_t)(u & 3) * 256 + lane4);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int RG, int D, bool SLOT, bool SADR>
__global__ void __launch_bounds__(256) ub44(const float* __restrict__ Wall, const float* __restrict__ X, float* __restrict__ Y, int L, int n_chains) {
  __shared__ __attribute__((aligned(16))) float xs[2 * 4 * RG * LDX];
  constexpr int R = 4 * RG;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = SADR ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int chain = blockIdx.x % 8, slice = blockIdx.x / 8;
  if (chain >= n_chains) return;
  const int row0 = slice * R;
  for (int e = tid; e < R * (W / 4); e += 256) {
    const int r = e / (W / 4), c4 = e % (W / 4);
    *(f32x4*)(&xs[r * LDX + 4 * c4]) = *(const f32x4*)(X + (size_t)(row0 + r) * W + 4 * c4);
  }
  const int n = wave * 64 + lane, lane4 = lane * 4;
  const float* w0 = Wall + (size_t)chain * L * W * W + (size_t)wave * KS * 256;   // [layer][tile][k4][lane][4]
  WStr ws;
#pragma unroll
  for (int u = 0; u < kPD; ++u) ws.b[u] = gload4(w0 + (size_t)u * 256 + lane4);
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const float* wp = w0 + (size_t)l * W * W;
    const int cur = (l & 1) * R * LDX, nxt = ((l + 1) & 1) * R * LDX;
    f32x4 acc[RG][2];
#pragma unroll
    for (int g = 0; g < RG; ++g) { acc[g][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[g][1] = acc[g][0]; }
    seg<RG, D, SLOT, SADR>(ws, wp, wp + (size_t)W * W, l + 1 < L, xs, cur + (lane & 3) * LDX, lane4, acc);
    float* yg = Y + ((size_t)chain * L + l) * 4096 * W;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      const f32x4 h = (acc[g][0] + acc[g][1]) * 0.05f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xs[nxt + (4 * g + r) * LDX + n] = h[r];
        yg[(size_t)(row0 + 4 * g + r) * W + n] = h[r];
      }
    }
    __syncthreads();
  }
}

template <typename F> float time_us(hipStream_t st, F launch, int reps) {
  for (int i = 0; i < 20; ++i) launch();
  hipStreamSynchronize(st);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0, st);
  for (int i = 0; i < reps; ++i) launch();
  hipEventRecord(e1, st);
  hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return ms * 1000.f / reps;
}

struct Variant { const char* name; void (*k)(const float*, const float*, float*, int, int); std::vector<float> per_layer; };

int main(int argc, char** argv) {
  const int n_chains = argc > 1 ? atoi(argv[1]) : 4;
  const int slices = argc > 2 ? atoi(argv[2]) : 32;
  const int rounds = argc > 3 ? atoi(argv[3]) : 3;
  const int LMAX = 9;
  hipStream_t st; CHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  float *Wd, *Xd, *Yd;
  const size_t nW = (size_t)8 * (LMAX + 1) * W * W;   // + one layer: the spare refills of the last trip stay inside the allocation
  CHK(hipMalloc(&Wd, nW * 4)); CHK(hipMalloc(&Xd, 4096 * W * 4)); CHK(hipMalloc(&Yd, (size_t)8 * LMAX * 4096 * W * 4));
  std::vector<float> hw(nW), hx(4096 * W);
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xFFFF) / 65536.0f - 0.5f; };
  for (auto& v : hw) v = rnd();
  for (auto& v : hx) v = rnd();
  CHK(hipMemcpy(Wd, hw.data(), nW * 4, hipMemcpyHostToDevice));
  CHK(hipMemcpy(Xd, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
  const int grid = 8 * slices;
  printf("4x4x1 chain step: chains %d, slices %d (%d workgroups), %d rounds; per layer us: min / median / max\n", n_chains, slices,
         n_chains * slices, rounds);
  std::vector<Variant> vs;
#define V(RG, D, SLOT, SADR) vs.push_back({"R=" #RG "x4 D=" #D " slot=" #SLOT " sadr=" #SADR, ub44<RG, D, SLOT, SADR>, {}})
#define VD(RG, SLOT, SADR) V(RG, 1, SLOT, SADR); V(RG, 2, SLOT, SADR); V(RG, 3, SLOT, SADR); V(RG, 4, SLOT, SADR)
  VD(1, false, false); VD(1, false, true); VD(1, true, false); VD(1, true, true);
  VD(2, false, false); VD(2, false, true);
  VD(4, false, false); VD(4, false, true);
  for (int r = 0; r < rounds; ++r)
    for (auto& v : vs) {
      float t3 = time_us(st, [&]() { hipLaunchKernelGGL(v.k, dim3(grid), dim3(256), 0, st, Wd, Xd, Yd, 3, n_chains); }, 200);
      float t9 = time_us(st, [&]() { hipLaunchKernelGGL(v.k, dim3(grid), dim3(256), 0, st, Wd, Xd, Yd, 9, n_chains); }, 200);
      CHK(hipGetLastError());
      v.per_layer.push_back((t9 - t3) / 6.0f);
    }
  for (auto& v : vs) {
    std::sort(v.per_layer.begin(), v.per_layer.end());
    const float md = v.per_layer[v.per_layer.size() / 2];
    printf("  %-34s %6.3f / %6.3f / %6.3f   = %5.1f cycles per step at 2.4 GHz\n", v.name, v.per_layer.front(), md, v.per_layer.back(),
           md * 2400.f / KS);
  }
  // correctness of layers 0 and 1 (chain 0, slice 0) for every variant: y1 = 0.05 * X . W0^T, y2 = 0.05 * y1 . W1^T, all variants bit-equal
  std::vector<float> y0;
  double md = 0;
  int differ = 0;
  for (auto& v : vs) {
    const int R = v.name[2] == '1' ? 4 : v.name[2] == '2' ? 8 : 16;
    CHK(hipMemsetAsync(Yd, 0, (size_t)2 * 4096 * W * 4, st));
    hipLaunchKernelGGL(v.k, dim3(grid), dim3(256), 0, st, Wd, Xd, Yd, 2, n_chains);
    CHK(hipStreamSynchronize(st));
    std::vector<float> y((size_t)(4096 + 4) * W);
    CHK(hipMemcpy(y.data(), Yd, y.size() * 4, hipMemcpyDeviceToHost));
    if (y0.empty()) {
      y0 = y;
      for (int l = 0; l < 2; ++l)
        for (int r = 0; r < 4; ++r)
          for (int n = 0; n < W; ++n) {
            double ref = 0;
            for (int k = 0; k < W; ++k)
              ref += (double)(l ? y[r * W + k] : hx[r * W + k]) * (double)hw[(size_t)l * W * W + ((size_t)(n / 64) * 64 + (k / 4)) * 256 + (n % 64) * 4 + (k % 4)];
            md = fmax(md, fabs(ref * 0.05 - (double)y[(size_t)l * 4096 * W + r * W + n]));
          }
    }
    for (int l = 0; l < 2; ++l)
      for (int i = 0; i < 4 * W; ++i) differ += y[(size_t)l * 4096 * W + i] != y0[(size_t)l * 4096 * W + i];
    (void)R;
  }
  printf("layers 0, 1 vs host (rows 0-3): max |diff| %.3g; elements that differ between variants: %d\n", md, differ);
  return differ != 0;
}
