// Fused LayerNorm forward/backward for gfx950 (CDNA4), bf16 activations,
// f32 affine parameters and f32 row statistics.
//
// Layout: x is [N, D] row-major bf16, D % 8 == 0.  One 64-lane wave owns one
// row (WAVES_PER_BLOCK rows per 256-thread workgroup), each lane streams the
// row as short8 (16 B) vector loads — the memory-bound regime for this op
// (guide Appendix B: elementwise/reduction; G13 vectorization).
//
// Capability parity note: the reference package has no kernels of its own
// (SURVEY.md §2.1); this op belongs to the framework's learned-test-classifier
// lane (transformer encoder LayerNorm).

#include "common.h"
#include "launchers.h"
#include <cstdlib>
#include <cstring>

#define WAVES_PER_BLOCK 4
#define BLOCK (WAVES_PER_BLOCK * WAVE)
// Register-resident row cache: up to 32 bf16x8 packets per lane = D <= 16384.
// The classifier uses D in {256,1024,2048}; loops below cap at D<=4096 for the
// cached path and re-read for larger D.
#define MAX_PKT 8  // cached path handles D <= 64*8*MAX_PKT = 4096

extern "C" {

__global__ void __launch_bounds__(BLOCK)
ln_fwd_kernel(const short* __restrict__ x, const short* __restrict__ res,
              const short* __restrict__ gamma,
              const short* __restrict__ beta, short* __restrict__ y,
              short* __restrict__ s_out,
              float* __restrict__ mean_out, float* __restrict__ rstd_out,
              int N, int D, float eps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int pkts = D / (WAVE * 8);  // short8 packets per lane (D % 512 == 0 fast path)
  for (int row = blockIdx.x * WAVES_PER_BLOCK + wid; row < N;
       row += gridDim.x * WAVES_PER_BLOCK) {
    const short* xr = x + (long)row * D;
    const short* rr = res ? res + (long)row * D : nullptr;
    short* yr = y + (long)row * D;
    short* sr = s_out ? s_out + (long)row * D : nullptr;
    float vals[MAX_PKT * 8];
    float s = 0.f;
    if (pkts <= MAX_PKT && D == pkts * WAVE * 8) {
#pragma unroll
      for (int p = 0; p < MAX_PKT; ++p) {
        if (p >= pkts) break;
        int base = (p * WAVE + lane) * 8;
        short8_t v = *(const short8_t*)(xr + base);
        short8_t so;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = bf16_to_f32(v[j]);
          vals[p * 8 + j] = f;
        }
        if (rr) {
          short8_t rv = *(const short8_t*)(rr + base);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            // bf16-rounded sum so s_out, the saved x for bwd, and the stats
            // all see the SAME residual-stream value
            short sum_b = f32_to_bf16(vals[p * 8 + j] + bf16_to_f32(rv[j]));
            vals[p * 8 + j] = bf16_to_f32(sum_b);
            so[j] = sum_b;
          }
          *(short8_t*)(sr + base) = so;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s += vals[p * 8 + j];
      }
      float mean = wave_sum(s) / (float)D;
      float var = 0.f;
#pragma unroll
      for (int p = 0; p < MAX_PKT; ++p) {
        if (p >= pkts) break;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float d = vals[p * 8 + j] - mean;
          var += d * d;
        }
      }
      var = wave_sum(var) / (float)D;
      float rstd = rsqrtf(var + eps);
      if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
      for (int p = 0; p < MAX_PKT; ++p) {
        if (p >= pkts) break;
        int base = (p * WAVE + lane) * 8;
        short8_t g8 = *(const short8_t*)(gamma + base);
        short8_t b8 = *(const short8_t*)(beta + base);
        short8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = (vals[p * 8 + j] - mean) * rstd;
          o[j] = f32_to_bf16(xhat * bf16_to_f32(g8[j]) + bf16_to_f32(b8[j]));
        }
        *(short8_t*)(yr + base) = o;
      }
    } else {
      // general path: two passes over the row, 8-wide loads, any D % 8 == 0
      for (int i = lane * 8; i < D; i += WAVE * 8) {
        short8_t v = *(const short8_t*)(xr + i);
        if (rr) {
          short8_t rv = *(const short8_t*)(rr + i);
          short8_t so;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            so[j] = f32_to_bf16(bf16_to_f32(v[j]) + bf16_to_f32(rv[j]));
          }
          *(short8_t*)(sr + i) = so;
          v = so;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) s += bf16_to_f32(v[j]);
      }
      float mean = wave_sum(s) / (float)D;
      float var = 0.f;
      for (int i = lane * 8; i < D; i += WAVE * 8) {
        short8_t v = *(const short8_t*)((rr ? sr : xr) + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float d = bf16_to_f32(v[j]) - mean;
          var += d * d;
        }
      }
      var = wave_sum(var) / (float)D;
      float rstd = rsqrtf(var + eps);
      if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
      for (int i = lane * 8; i < D; i += WAVE * 8) {
        short8_t v = *(const short8_t*)((rr ? sr : xr) + i);
        short8_t g8 = *(const short8_t*)(gamma + i);
        short8_t b8 = *(const short8_t*)(beta + i);
        short8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xhat = (bf16_to_f32(v[j]) - mean) * rstd;
          o[j] = f32_to_bf16(xhat * bf16_to_f32(g8[j]) + bf16_to_f32(b8[j]));
        }
        *(short8_t*)(yr + i) = o;
      }
    }
  }
}

}  // extern "C" (templates below need C++ linkage)

// Template-specialized fast path: exact unroll for D = PKTS*512 (no
// MAX_PKT-sized register waste), gamma/beta hoisted out of the row loop,
// and the NEXT row's packets prefetched before the wave-reduction chains so
// the loads overlap the two log2(64) shuffle reductions.  One wave per row.
template <int PKTS, bool HASRES>
__global__ void __launch_bounds__(BLOCK)
ln_fwd_t(const short* __restrict__ x, const short* __restrict__ res,
         const short* __restrict__ gamma, const short* __restrict__ beta,
         short* __restrict__ y, short* __restrict__ s_out,
         float* __restrict__ mean_out, float* __restrict__ rstd_out,
         int N, int D, float eps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int rstride = gridDim.x * WAVES_PER_BLOCK;
  int row = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (row >= N) return;
  float gv[PKTS * 8], bv[PKTS * 8];
#pragma unroll
  for (int p = 0; p < PKTS; ++p) {
    int base = (p * WAVE + lane) * 8;
    short8_t g8 = *(const short8_t*)(gamma + base);
    short8_t b8 = *(const short8_t*)(beta + base);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      gv[p * 8 + j] = bf16_to_f32(g8[j]);
      bv[p * 8 + j] = bf16_to_f32(b8[j]);
    }
  }
  short8_t vx[PKTS], vr[PKTS];
#pragma unroll
  for (int p = 0; p < PKTS; ++p) {
    int base = (p * WAVE + lane) * 8;
    vx[p] = *(const short8_t*)(x + (long)row * D + base);
    if (HASRES) vr[p] = *(const short8_t*)(res + (long)row * D + base);
  }
  while (true) {
    const int next = row + rstride;
    float vals[PKTS * 8];
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
      short8_t so;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_to_f32(vx[p][j]);
        if (HASRES) {
          // bf16-rounded sum so s_out, the saved x for bwd, and the stats
          // all see the SAME residual-stream value
          short sum_b = f32_to_bf16(f + bf16_to_f32(vr[p][j]));
          f = bf16_to_f32(sum_b);
          so[j] = sum_b;
        }
        vals[p * 8 + j] = f;
        s += f;
      }
      if (HASRES)
        *(short8_t*)(s_out + (long)row * D + (p * WAVE + lane) * 8) = so;
    }
    if (next < N) {
#pragma unroll
      for (int p = 0; p < PKTS; ++p) {
        int base = (p * WAVE + lane) * 8;
        vx[p] = *(const short8_t*)(x + (long)next * D + base);
        if (HASRES) vr[p] = *(const short8_t*)(res + (long)next * D + base);
      }
    }
    float mean = wave_sum(s) / (float)D;
    float var = 0.f;
#pragma unroll
    for (int k = 0; k < PKTS * 8; ++k) {
      float d = vals[k] - mean;
      var += d * d;
    }
    var = wave_sum(var) / (float)D;
    float rstd = rsqrtf(var + eps);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
      short8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = p * 8 + j;
        o[j] = f32_to_bf16((vals[k] - mean) * rstd * gv[k] + bv[k]);
      }
      *(short8_t*)(y + (long)row * D + (p * WAVE + lane) * 8) = o;
    }
    if (next >= N) break;
    row = next;
  }
}

// Column partials of the LayerNorm backward.  Every backward kernel writes
// ONE f32 workspace row of NOUT * D floats per block (per wave on the wide
// path): [dgamma | dbeta] and, with DRES, a third slab [dres_sum] — the
// column sum of the bf16-rounded dx values the kernel stores, which is the
// bias gradient of the projection that fed this LayerNorm's residual input.
// A single colsum chain over width NOUT * D then reduces all of them.
//
// Fixed-order merge of a block's four waves through LDS, wave 0 first: every
// column is summed in the same order on every run, with no atomics (an
// LDS-atomicAdd merge was caught non-deterministic by
// test_kernels_bitwise_deterministic).  Lane l owns columns
// (p * 64 + l) * 8 + j of every slab; all four barriers are block-uniform.
template <int PKTS, int NOUT>
__device__ __forceinline__ void ln_bwd_merge_store(
    const float (&acc)[NOUT][PKTS * 8], float* __restrict__ sm,
    float* __restrict__ ws, int lane, int wid) {
  constexpr int DT = PKTS * WAVE * 8;
  for (int w = 0; w < WAVES_PER_BLOCK; ++w) {
    if (wid == w) {
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
#pragma unroll
        for (int p = 0; p < PKTS; ++p) {
          float4_t* s4 = (float4_t*)(sm + o * DT + (p * WAVE + lane) * 8);
          float4_t a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
          if (w) { a = s4[0]; b = s4[1]; }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            a[j] += acc[o][p * 8 + j];
            b[j] += acc[o][p * 8 + 4 + j];
          }
          s4[0] = a; s4[1] = b;
        }
      }
    }
    __syncthreads();
  }
  float* orow = ws + (long)blockIdx.x * (NOUT * DT);
  for (int i = threadIdx.x * 4; i < NOUT * DT; i += BLOCK * 4)
    *(float4_t*)(orow + i) = *(const float4_t*)(sm + i);
}

// One row per wave; partials accumulate in registers (each (wave, lane, j)
// owns a fixed column set) and merge per block as above.  ws has gridDim.x
// rows; the colsum reduces them in fixed order.
template <int PKTS, bool HASDE, bool DRES>
__global__ void __launch_bounds__(BLOCK)
ln_bwd_t(const short* __restrict__ dy, const short* __restrict__ x,
         const short* __restrict__ gamma, const float* __restrict__ mean_in,
         const float* __restrict__ rstd_in,
         const short* __restrict__ ds_extra, short* __restrict__ dx,
         float* __restrict__ ws, int N, int D) {
  constexpr int NOUT = DRES ? 3 : 2;
  __shared__ __attribute__((aligned(16))) float sm[NOUT * PKTS * WAVE * 8];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  float gv[PKTS * 8];
#pragma unroll
  for (int p = 0; p < PKTS; ++p) {
    short8_t g8 = *(const short8_t*)(gamma + (p * WAVE + lane) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) gv[p * 8 + j] = bf16_to_f32(g8[j]);
  }
  float acc[NOUT][PKTS * 8] = {{0.f}};  // [dgamma, dbeta, dres_sum]
  const int rstride = gridDim.x * WAVES_PER_BLOCK;
  int row = blockIdx.x * WAVES_PER_BLOCK + wid;
  const bool active = row < N;
  short8_t vd[PKTS], vxp[PKTS], ve[PKTS];
  if (active) {
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
      int base = (p * WAVE + lane) * 8;
      vd[p] = *(const short8_t*)(dy + (long)row * D + base);
      vxp[p] = *(const short8_t*)(x + (long)row * D + base);
      if (HASDE) ve[p] = *(const short8_t*)(ds_extra + (long)row * D + base);
    }
  }
  while (active) {
    const int next = row + rstride;
    const float mean = mean_in[row], rstd = rstd_in[row];
    float xh[PKTS * 8], dyg[PKTS * 8], ev[PKTS * 8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = p * 8 + j;
        float d = bf16_to_f32(vd[p][j]);
        float h = (bf16_to_f32(vxp[p][j]) - mean) * rstd;
        float g = d * gv[k];
        if (HASDE) ev[k] = bf16_to_f32(ve[p][j]);
        xh[k] = h; dyg[k] = g;
        acc[0][k] += d * h;
        acc[1][k] += d;
        s1 += g; s2 += g * h;
      }
    }
    if (next < N) {
#pragma unroll
      for (int p = 0; p < PKTS; ++p) {
        int base = (p * WAVE + lane) * 8;
        vd[p] = *(const short8_t*)(dy + (long)next * D + base);
        vxp[p] = *(const short8_t*)(x + (long)next * D + base);
        if (HASDE) ve[p] = *(const short8_t*)(ds_extra + (long)next * D + base);
      }
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
      short8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = p * 8 + j;
        float d_ = rstd * (dyg[k] - s1 - xh[k] * s2);
        if (HASDE) d_ += ev[k];
        o[j] = f32_to_bf16(d_);
        // the sum of what is STORED: round first, then accumulate
        if (DRES) acc[NOUT - 1][k] += bf16_to_f32(o[j]);
      }
      *(short8_t*)(dx + (long)row * D + (p * WAVE + lane) * 8) = o;
    }
    if (next >= N) break;
    row = next;
  }
  ln_bwd_merge_store<PKTS, NOUT>(acc, sm, ws, lane, wid);
}

// Two rows per wave (round 2): the single-row ln_bwd_t is latency-bound on
// its serial chain (2 dependent wave_sum shuffle reductions + the dx store
// per row; measured ~2-3 TB/s vs ln_fwd's 6.4).  Interleaving two
// independent rows per wave doubles the work inside the same latency
// shadow — the four wave_sum chains (s1/s2 x 2 rows) issue back-to-back.
// The column accumulators are shared (summed over both rows, row A first), so
// the workspace layout and the deterministic colsum are unchanged.
template <int PKTS, bool HASDE, bool DRES>
__global__ void __launch_bounds__(BLOCK)
ln_bwd_t2(const short* __restrict__ dy, const short* __restrict__ x,
          const short* __restrict__ gamma, const float* __restrict__ mean_in,
          const float* __restrict__ rstd_in,
          const short* __restrict__ ds_extra, short* __restrict__ dx,
          float* __restrict__ ws, int N, int D) {
  constexpr int NOUT = DRES ? 3 : 2;
  __shared__ __attribute__((aligned(16))) float sm[NOUT * PKTS * WAVE * 8];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  float gv[PKTS * 8];
#pragma unroll
  for (int p = 0; p < PKTS; ++p) {
    short8_t g8 = *(const short8_t*)(gamma + (p * WAVE + lane) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) gv[p * 8 + j] = bf16_to_f32(g8[j]);
  }
  float acc[NOUT][PKTS * 8] = {{0.f}};  // [dgamma, dbeta, dres_sum]
  const int rstride = gridDim.x * WAVES_PER_BLOCK * 2;
  int rowA = (blockIdx.x * WAVES_PER_BLOCK + wid) * 2;
  short8_t vdA[PKTS], vxA[PKTS], veA[PKTS];
  short8_t vdB[PKTS], vxB[PKTS], veB[PKTS];
  bool actA = rowA < N, actB = rowA + 1 < N;
  if (actA) {
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
      int base = (p * WAVE + lane) * 8;
      vdA[p] = *(const short8_t*)(dy + (long)rowA * D + base);
      vxA[p] = *(const short8_t*)(x + (long)rowA * D + base);
      if (HASDE) veA[p] = *(const short8_t*)(ds_extra + (long)rowA * D + base);
      if (actB) {
        vdB[p] = *(const short8_t*)(dy + (long)(rowA + 1) * D + base);
        vxB[p] = *(const short8_t*)(x + (long)(rowA + 1) * D + base);
        if (HASDE)
          veB[p] = *(const short8_t*)(ds_extra + (long)(rowA + 1) * D + base);
      }
    }
  }
  while (actA) {
    const int next = rowA + rstride;
    const float meanA = mean_in[rowA], rstdA = rstd_in[rowA];
    const float meanB = actB ? mean_in[rowA + 1] : 0.f;
    const float rstdB = actB ? rstd_in[rowA + 1] : 0.f;
    float xhA[PKTS * 8], dygA[PKTS * 8];
    float xhB[PKTS * 8], dygB[PKTS * 8];
    float s1A = 0.f, s2A = 0.f, s1B = 0.f, s2B = 0.f;
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = p * 8 + j;
        float dA = bf16_to_f32(vdA[p][j]);
        float hA = (bf16_to_f32(vxA[p][j]) - meanA) * rstdA;
        float gA = dA * gv[k];
        xhA[k] = hA; dygA[k] = gA;
        acc[0][k] += dA * hA;
        acc[1][k] += dA;
        s1A += gA; s2A += gA * hA;
        if (actB) {
          float dB = bf16_to_f32(vdB[p][j]);
          float hB = (bf16_to_f32(vxB[p][j]) - meanB) * rstdB;
          float gB = dB * gv[k];
          xhB[k] = hB; dygB[k] = gB;
          acc[0][k] += dB * hB;
          acc[1][k] += dB;
          s1B += gB; s2B += gB * hB;
        }
      }
    }
    if (next < N) {
#pragma unroll
      for (int p = 0; p < PKTS; ++p) {
        int base = (p * WAVE + lane) * 8;
        vdA[p] = *(const short8_t*)(dy + (long)next * D + base);
        vxA[p] = *(const short8_t*)(x + (long)next * D + base);
        if (next + 1 < N) {
          vdB[p] = *(const short8_t*)(dy + (long)(next + 1) * D + base);
          vxB[p] = *(const short8_t*)(x + (long)(next + 1) * D + base);
        }
      }
    }
    s1A = wave_sum(s1A) / (float)D;
    s2A = wave_sum(s2A) / (float)D;
    if (actB) {
      s1B = wave_sum(s1B) / (float)D;
      s2B = wave_sum(s2B) / (float)D;
    }
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
      short8_t oA, oB;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = p * 8 + j;
        float dA_ = rstdA * (dygA[k] - s1A - xhA[k] * s2A);
        if (HASDE) dA_ += bf16_to_f32(veA[p][j]);
        oA[j] = f32_to_bf16(dA_);
        // the sum of what is STORED: round first, then accumulate
        if (DRES) acc[NOUT - 1][k] += bf16_to_f32(oA[j]);
        if (actB) {
          float dB_ = rstdB * (dygB[k] - s1B - xhB[k] * s2B);
          if (HASDE) dB_ += bf16_to_f32(veB[p][j]);
          oB[j] = f32_to_bf16(dB_);
          if (DRES) acc[NOUT - 1][k] += bf16_to_f32(oB[j]);
        }
      }
      int base = (p * WAVE + lane) * 8;
      *(short8_t*)(dx + (long)rowA * D + base) = oA;
      if (actB) *(short8_t*)(dx + (long)(rowA + 1) * D + base) = oB;
    }
    if (next >= N) break;
    rowA = next;
    actB = rowA + 1 < N;
    if (HASDE) {
#pragma unroll
      for (int p = 0; p < PKTS; ++p) {
        int base = (p * WAVE + lane) * 8;
        veA[p] = *(const short8_t*)(ds_extra + (long)rowA * D + base);
        if (actB)
          veB[p] = *(const short8_t*)(ds_extra + (long)(rowA + 1) * D + base);
      }
    }
  }
  ln_bwd_merge_store<PKTS, NOUT>(acc, sm, ws, lane, wid);
}

// General-width backward, any D % 8 == 0 up to MAXP * 512 (the widths
// without an ln_bwd_t2 instance: 128, 256, 2048, 4096, odd ones like 136).
//   dx = rstd * (dyg - mean(dyg) - xhat * mean(dyg * xhat)),  dyg = dy * gamma
// One wave per row; lane l owns columns (p * 64 + l) * 8 + j for its whole
// row loop, so the row and the dgamma/dbeta partials stay in registers.
// The four waves of a block then merge their partials through LDS one wave
// at a time, wave 0 first: every column is summed in the same order on
// every run, with no atomics.  One ws row of NOUT * D floats per block.
template <int MAXP, bool DRES>
__global__ void __launch_bounds__(BLOCK)
ln_bwd_g(const short* __restrict__ dy, const short* __restrict__ x,
         const short* __restrict__ gamma, const float* __restrict__ mean_in,
         const float* __restrict__ rstd_in,
         const short* __restrict__ ds_extra,  // optional += into dx
         short* __restrict__ dx, float* __restrict__ ws, int N, int D) {
  constexpr int NOUT = DRES ? 3 : 2;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm = (float*)smem;  // [NOUT, D] partials of this block
  float acc[NOUT][MAXP * 8] = {{0.f}};  // [dgamma, dbeta, dres_sum]
  for (int row = blockIdx.x * WAVES_PER_BLOCK + wid; row < N;
       row += gridDim.x * WAVES_PER_BLOCK) {
    const short* dyr = dy + (long)row * D;
    const short* xr = x + (long)row * D;
    const short* der = ds_extra ? ds_extra + (long)row * D : nullptr;
    short* dxr = dx + (long)row * D;
    const float mean = mean_in[row], rstd = rstd_in[row];
    short8_t vd[MAXP], vx[MAXP], vg[MAXP];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      int base = (p * WAVE + lane) * 8;
      if (base >= D) continue;
      vd[p] = *(const short8_t*)(dyr + base);
      vx[p] = *(const short8_t*)(xr + base);
      vg[p] = *(const short8_t*)(gamma + base);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = bf16_to_f32(vd[p][j]);
        float h = (bf16_to_f32(vx[p][j]) - mean) * rstd;
        float g = d * bf16_to_f32(vg[p][j]);
        acc[0][p * 8 + j] += d * h;
        acc[1][p * 8 + j] += d;
        s1 += g; s2 += g * h;
      }
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      int base = (p * WAVE + lane) * 8;
      if (base >= D) continue;
      short8_t ev;
      if (der) ev = *(const short8_t*)(der + base);
      short8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float h = (bf16_to_f32(vx[p][j]) - mean) * rstd;
        float g = bf16_to_f32(vd[p][j]) * bf16_to_f32(vg[p][j]);
        float d_ = rstd * (g - s1 - h * s2);
        if (der) d_ += bf16_to_f32(ev[j]);
        o[j] = f32_to_bf16(d_);
        // the sum of what is STORED: round first, then accumulate
        if (DRES) acc[NOUT - 1][p * 8 + j] += bf16_to_f32(o[j]);
      }
      *(short8_t*)(dxr + base) = o;
    }
  }
  // fixed-order merge: wave w adds its partials after waves 0..w-1 have
  // (a wave without rows adds zeros); all four barriers are block-uniform
  for (int w = 0; w < WAVES_PER_BLOCK; ++w) {
    if (wid == w) {
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
#pragma unroll
        for (int p = 0; p < MAXP; ++p) {
          int base = (p * WAVE + lane) * 8;
          if (base >= D) continue;
          float* so = sm + o * D;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float prev = w ? so[base + j] : 0.f;
            so[base + j] = prev + acc[o][p * 8 + j];
          }
        }
      }
    }
    __syncthreads();
  }
  float* orow = ws + (long)blockIdx.x * (NOUT * D);
  for (int i = threadIdx.x; i < NOUT * D; i += BLOCK) orow[i] = sm[i];
}

// Widths above LN_BWD_G_MAX_D: the partials no longer fit in registers, so
// every wave accumulates into its OWN ws row in global memory (the lane that
// owns a column is the only one that ever touches it: plain read-add-write,
// no atomics), and the colsum reduces the gridDim.x * WAVES_PER_BLOCK rows in
// fixed order like the template path's.
#define LN_BWD_G_MAX_D 4096
template <bool DRES>
__global__ void __launch_bounds__(BLOCK)
ln_bwd_wide_kernel(const short* __restrict__ dy, const short* __restrict__ x,
                   const short* __restrict__ gamma,
                   const float* __restrict__ mean_in,
                   const float* __restrict__ rstd_in,
                   const short* __restrict__ ds_extra,
                   short* __restrict__ dx, float* __restrict__ ws, int N,
                   int D) {
  constexpr int NOUT = DRES ? 3 : 2;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  float* og = ws + (long)(blockIdx.x * WAVES_PER_BLOCK + wid) * (NOUT * D);
  float* ob = og + D;
  float* od = og + (NOUT - 1) * D;  // dres_sum slab (DRES only)
  for (int i = lane * 8; i < D; i += WAVE * 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      og[i + j] = 0.f; ob[i + j] = 0.f;
      if (DRES) od[i + j] = 0.f;
    }
  }
  for (int row = blockIdx.x * WAVES_PER_BLOCK + wid; row < N;
       row += gridDim.x * WAVES_PER_BLOCK) {
    const short* dyr = dy + (long)row * D;
    const short* xr = x + (long)row * D;
    const short* der = ds_extra ? ds_extra + (long)row * D : nullptr;
    short* dxr = dx + (long)row * D;
    const float mean = mean_in[row], rstd = rstd_in[row];
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane * 8; i < D; i += WAVE * 8) {
      short8_t vd = *(const short8_t*)(dyr + i);
      short8_t vx = *(const short8_t*)(xr + i);
      short8_t g8 = *(const short8_t*)(gamma + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float g = bf16_to_f32(vd[j]) * bf16_to_f32(g8[j]);
        float h = (bf16_to_f32(vx[j]) - mean) * rstd;
        s1 += g; s2 += g * h;
      }
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
    for (int i = lane * 8; i < D; i += WAVE * 8) {
      short8_t vd = *(const short8_t*)(dyr + i);
      short8_t vx = *(const short8_t*)(xr + i);
      short8_t g8 = *(const short8_t*)(gamma + i);
      short8_t ev;
      if (der) ev = *(const short8_t*)(der + i);
      short8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = bf16_to_f32(vd[j]);
        float h = (bf16_to_f32(vx[j]) - mean) * rstd;
        float g = d * bf16_to_f32(g8[j]);
        float d_ = rstd * (g - s1 - h * s2);
        if (der) d_ += bf16_to_f32(ev[j]);
        o[j] = f32_to_bf16(d_);
        og[i + j] += d * h;
        ob[i + j] += d;
        if (DRES) od[i + j] += bf16_to_f32(o[j]);
      }
      *(short8_t*)(dxr + i) = o;
    }
  }
}

// Launch geometry.  Forward: one wave per row, grid-stride past the cap.
// Backward: the [rows, n_out * D] partials workspace and its column sum
// scale linearly with the grid, so it stays modest; D > LN_BWD_G_MAX_D keeps
// one workspace row per WAVE in global memory, hence a quarter of the grid.
#define LN_FWD_MAX_GRID 4096
#define LN_BWD_MAX_GRID 1024
static int ln_row_blocks(int N, int cap) {
  int blocks = (int)(((long)N + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
  return blocks < cap ? blocks : cap;
}
static int ln_bwd_grid(int N, int D) {
  return ln_row_blocks(N, D > LN_BWD_G_MAX_D ? LN_BWD_MAX_GRID / WAVES_PER_BLOCK
                                             : LN_BWD_MAX_GRID);
}

extern "C" {

hipError_t ln_fwd_launch(const void* x, const void* res, const void* gamma,
                         const void* beta, void* y, void* s_out, void* mean,
                         void* rstd, int N, int D, float eps,
                         hipStream_t stream) {
  const int grid = ln_row_blocks(N, LN_FWD_MAX_GRID);
#define LNF_T(P)                                                              \
  do {                                                                        \
    if (res)                                                                  \
      ln_fwd_t<P, true><<<grid, BLOCK, 0, stream>>>(                          \
          (const short*)x, (const short*)res, (const short*)gamma,            \
          (const short*)beta, (short*)y, (short*)s_out, (float*)mean,         \
          (float*)rstd, N, D, eps);                                           \
    else                                                                      \
      ln_fwd_t<P, false><<<grid, BLOCK, 0, stream>>>(                         \
          (const short*)x, nullptr, (const short*)gamma, (const short*)beta,  \
          (short*)y, (short*)s_out, (float*)mean, (float*)rstd, N, D, eps);   \
  } while (0)
  if (D == 512) LNF_T(1);
  else if (D == 1024) LNF_T(2);
  else if (D == 2048) LNF_T(4);
  // PKTS=8 (D=4096) allocates 256 VGPRs (1 wave/SIMD) — the general kernel
  // is the better trade there
  else
    ln_fwd_kernel<<<grid, BLOCK, 0, stream>>>(
        (const short*)x, (const short*)res, (const short*)gamma,
        (const short*)beta, (short*)y, (short*)s_out, (float*)mean,
        (float*)rstd, N, D, eps);
#undef LNF_T
  return hipGetLastError();
}

// runtime A/B: TOSEM_LN_BWD=1row selects the single-row ln_bwd_t variant
static int ln_bwd_use_1row() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("TOSEM_LN_BWD");
    v = (e && strcmp(e, "1row") == 0) ? 1 : 0;
  }
  return v;
}

// ws is [ln_bwd_ws_rows(N, D), n_out * D] f32 with n_out = 2
// ([dgamma | dbeta]) or 3 (+ [dres_sum]); every width supports both.
hipError_t ln_bwd_launch(const void* dy, const void* x, const void* gamma,
                         const void* mean, const void* rstd,
                         const void* ds_extra, void* dx, void* ws, int n_out,
                         int N, int D, hipStream_t stream) {
  if (n_out != 2 && n_out != 3) return hipErrorInvalidValue;
  const int grid = ln_bwd_grid(N, D);
  const bool dres = n_out == 3;
  size_t shm = (size_t)D * n_out * sizeof(float);
#define LNB_ARGS                                                              \
  (const short*)dy, (const short*)x, (const short*)gamma, (const float*)mean, \
      (const float*)rstd, (const short*)ds_extra, (short*)dx, (float*)ws, N, D
#define LNB_K(K, P)                                                           \
  do {                                                                        \
    if (ds_extra && dres) {                                                   \
      K<P, true, true><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);                 \
    } else if (ds_extra) {                                                    \
      K<P, true, false><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);                \
    } else if (dres) {                                                        \
      K<P, false, true><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);                \
    } else {                                                                  \
      K<P, false, false><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);               \
    }                                                                         \
  } while (0)
#define LNB_T(P)                                                              \
  do {                                                                        \
    if (ln_bwd_use_1row()) {                                                  \
      LNB_K(ln_bwd_t, P);                                                     \
    } else {                                                                  \
      LNB_K(ln_bwd_t2, P);                                                    \
    }                                                                         \
  } while (0)
#define LNB_G(P)                                                              \
  do {                                                                        \
    if (dres) {                                                               \
      ln_bwd_g<P, true><<<grid, BLOCK, shm, stream>>>(LNB_ARGS);              \
    } else {                                                                  \
      ln_bwd_g<P, false><<<grid, BLOCK, shm, stream>>>(LNB_ARGS);             \
    }                                                                         \
  } while (0)
  if (D == 512) LNB_T(1);
  else if (D == 1024) LNB_T(2);
  else if (D <= 512) LNB_G(1);
  else if (D <= 1024) LNB_G(2);
  else if (D <= 2048) LNB_G(4);
  else if (D <= LN_BWD_G_MAX_D) LNB_G(8);
  else if (dres) {
    ln_bwd_wide_kernel<true><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);
  } else {
    ln_bwd_wide_kernel<false><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);
  }
#undef LNB_G
#undef LNB_T
#undef LNB_K
#undef LNB_ARGS
  return hipGetLastError();
}

// Workspace rows ln_bwd_launch writes: one per block (the waves merge through
// LDS), one per wave on the wide path.  Either way the column sum reduces
// them in fixed order.
int ln_bwd_ws_rows(int N, int D) {
  const int grid = ln_bwd_grid(N, D);
  return D > LN_BWD_G_MAX_D ? grid * WAVES_PER_BLOCK : grid;
}

}  // extern "C"
