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
#include "mx.h"
#include "philox.h"
#include <cstdlib>
#include <cstring>

#define WAVES_PER_BLOCK 4
#define BLOCK (WAVES_PER_BLOCK * WAVE)
// Register-resident row cache: up to 32 bf16x8 packets per lane = D <= 16384.
// The classifier uses D in {256,1024,2048}; loops below cap at D<=4096 for the
// cached path and re-read for larger D.
#define MAX_PKT 8  // cached path handles D <= 64*8*MAX_PKT = 4096

// Fused residual dropout (DROP instantiations; docs/KERNELS.md "Fused
// residual dropout").  The keep bits of a packet come from drop_keep8
// (philox.h), indexed by the packet's GLOBAL element offset, so the mask is
// the same whatever the grid, the rows per wave or the kernel variant.
//
// Forward: the f32 stream value x + (keep ? res * scale : 0), which the
// caller rounds to bf16 once.  Contraction is off so that the product rounds
// to f32 before the add, as the reference's separate multiply and add do.
__device__ __forceinline__ float drop_add(float x, float r, bool keep,
                                          float scale) {
#pragma clang fp contract(off)
  float t = r * scale;
  return x + (keep ? t : 0.f);
}

// The rounding points of ln_bwd_t2's DROP instantiations, spelled out.
// Whether a product is fused into the add that follows it is otherwise the
// optimizer's choice per instantiation, and the dropout instantiations must
// return bit for bit the dx, dgamma and dbeta of their siblings, which
// compile to: column and row sums from rounded products (no fusing), dx from
// fused ones (ln_bwd_t2_dx below).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// dx = rstd * (dyg - s1 - xh * s2) [+ ds_extra], both products fused.
template <bool HASDE>
__device__ __forceinline__ float ln_bwd_t2_dx(float dyg, float xh, float s1,
                                              float s2, float rstd, short ve) {
  const float t = __builtin_fmaf(-xh, s2, dyg - s1);
  return HASDE ? __builtin_fmaf(rstd, t, bf16_to_f32(ve)) : rstd * t;
}

// Backward: dres = keep ? bf16(v * scale) : 0, v being the f32 value dx is
// rounded from.
__device__ __forceinline__ short drop_grad(float v, bool keep, float scale) {
  return keep ? f32_to_bf16(v * scale) : (short)0;
}

// MX output mode of the two forward kernels (inference; mx.h,
// docs/KERNELS.md "MXFP8 operands"): the normalised value is rounded to bf16
// in registers exactly as the bf16 mode stores it, and that packet is
// quantised instead of stored.  The bodies are shared, so the arithmetic
// order is.
//
// READ THIS before touching the MX instantiations: they keep the bf16
// kernels' parameter list, so that the bf16 instantiations compile to what
// they were, and two of its pointers carry other data under other types:
//
//   parameter           bf16 mode               MX mode
//   short* y            y [N, D] bf16           q [N, D] e4m3 BYTES
//   float* mean_out     mean [N] f32            scales [N, D / 32] e8m0 BYTES
//   float* rstd_out     rstd [N] f32            nullptr, never touched
//
// LnMxOut names the two under their real types, and every MX access goes
// through it; `y`, `mean_out` and `rstd_out` themselves are only
// dereferenced under !MX.  D % 32 == 0, so in the general path a lane quad
// enters or leaves the packet loop as a whole.
struct LnMxOut {
  unsigned char* q;       // [N, D] e4m3fn bytes
  unsigned char* scales;  // [N, D / 32] e8m0 bytes
};
__device__ __forceinline__ LnMxOut ln_mx_out(short* y, float* mean_out) {
  return LnMxOut{(unsigned char*)y, (unsigned char*)mean_out};
}

// One packet of the output: to dst (bf16 mode), or quantised to element
// offset elem of mx (MX mode).
template <bool MX>
__device__ __forceinline__ void ln_store_out(short8_t o, short* dst, long elem,
                                             LnMxOut mx) {
  if (MX)
    mx_store_packet(o, elem, mx.q, mx.scales);
  else
    *(short8_t*)dst = o;
}

template <bool DROP, bool MX>
__global__ void __launch_bounds__(BLOCK)
ln_fwd_kernel(const short* __restrict__ x, const short* __restrict__ res,
              const short* __restrict__ gamma,
              const short* __restrict__ beta, short* __restrict__ y,
              short* __restrict__ s_out,
              float* __restrict__ mean_out, float* __restrict__ rstd_out,
              int N, int D, float eps, LnDrop dr) {
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
          unsigned keep = 0;
          if (DROP) keep = drop_keep8(dr, ((long)row * D + base) >> 3);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            // bf16-rounded sum so s_out, the saved x for bwd, and the stats
            // all see the SAME residual-stream value
            float sum = DROP ? drop_add(vals[p * 8 + j], bf16_to_f32(rv[j]),
                                        (keep >> j) & 1, dr.scale)
                             : vals[p * 8 + j] + bf16_to_f32(rv[j]);
            short sum_b = f32_to_bf16(sum);
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
      if (!MX && lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
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
        ln_store_out<MX>(o, yr + base, (long)row * D + base,
                         ln_mx_out(y, mean_out));
      }
    } else {
      // general path: two passes over the row, 8-wide loads, any D % 8 == 0
      for (int i = lane * 8; i < D; i += WAVE * 8) {
        short8_t v = *(const short8_t*)(xr + i);
        if (rr) {
          short8_t rv = *(const short8_t*)(rr + i);
          short8_t so;
          unsigned keep = 0;
          if (DROP) keep = drop_keep8(dr, ((long)row * D + i) >> 3);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float sum = DROP ? drop_add(bf16_to_f32(v[j]), bf16_to_f32(rv[j]),
                                        (keep >> j) & 1, dr.scale)
                             : bf16_to_f32(v[j]) + bf16_to_f32(rv[j]);
            so[j] = f32_to_bf16(sum);
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
      if (!MX && lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
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
        ln_store_out<MX>(o, yr + i, (long)row * D + i,
                         ln_mx_out(y, mean_out));
      }
    }
  }
}

// Template-specialized fast path: exact unroll for D = PKTS*512 (no
// MAX_PKT-sized register waste), gamma/beta hoisted out of the row loop,
// and the NEXT row's packets prefetched before the wave-reduction chains so
// the loads overlap the two log2(64) shuffle reductions.  One wave per row.
template <int PKTS, bool HASRES, bool DROP, bool MX>
__global__ void __launch_bounds__(BLOCK)
ln_fwd_t(const short* __restrict__ x, const short* __restrict__ res,
         const short* __restrict__ gamma, const short* __restrict__ beta,
         short* __restrict__ y, short* __restrict__ s_out,
         float* __restrict__ mean_out, float* __restrict__ rstd_out,
         int N, int D, float eps, LnDrop dr) {
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
      unsigned keep = 0;
      if (DROP)
        keep = drop_keep8(dr, ((long)row * D + (p * WAVE + lane) * 8) >> 3);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_to_f32(vx[p][j]);
        if (HASRES) {
          // bf16-rounded sum so s_out, the saved x for bwd, and the stats
          // all see the SAME residual-stream value
          float sum = DROP ? drop_add(f, bf16_to_f32(vr[p][j]),
                                      (keep >> j) & 1, dr.scale)
                           : f + bf16_to_f32(vr[p][j]);
          short sum_b = f32_to_bf16(sum);
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
    if (!MX && lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
    for (int p = 0; p < PKTS; ++p) {
      short8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = p * 8 + j;
        o[j] = f32_to_bf16((vals[k] - mean) * rstd * gv[k] + bv[k]);
      }
      const long elem = (long)row * D + (p * WAVE + lane) * 8;
      ln_store_out<MX>(o, y + elem, elem, ln_mx_out(y, mean_out));
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
// DROP: a second output dres, the gradient of the dropped residual input
// (drop_grad above); dx, the partials and their order are untouched.
template <int PKTS, bool HASDE, bool DRES, bool DROP>
__global__ void __launch_bounds__(BLOCK)
ln_bwd_t2(const short* __restrict__ dy, const short* __restrict__ x,
          const short* __restrict__ gamma, const float* __restrict__ mean_in,
          const float* __restrict__ rstd_in,
          const short* __restrict__ ds_extra, short* __restrict__ dx,
          float* __restrict__ ws, int N, int D, short* __restrict__ dres,
          LnDrop dr) {
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
        float gA = DROP ? mul_rn(dA, gv[k]) : dA * gv[k];
        xhA[k] = hA; dygA[k] = gA;
        acc[0][k] += DROP ? mul_rn(dA, hA) : dA * hA;
        acc[1][k] += dA;
        s1A += gA; s2A += DROP ? mul_rn(gA, hA) : gA * hA;
        if (actB) {
          float dB = bf16_to_f32(vdB[p][j]);
          float hB = (bf16_to_f32(vxB[p][j]) - meanB) * rstdB;
          float gB = DROP ? mul_rn(dB, gv[k]) : dB * gv[k];
          xhB[k] = hB; dygB[k] = gB;
          acc[0][k] += DROP ? mul_rn(dB, hB) : dB * hB;
          acc[1][k] += dB;
          s1B += gB; s2B += DROP ? mul_rn(gB, hB) : gB * hB;
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
      const int base = (p * WAVE + lane) * 8;
      if (DROP) {
        // one row after the other: the Philox state and the second output
        // vector of both rows at once cost the D = 1024 instance a wave
        // per SIMD (docs/KERNELS.md)
        auto emit = [&](int row, const float* dyg, const float* xh,
                        const short8_t& ve, float rstd, float s1, float s2) {
          const unsigned keep = drop_keep8(dr, ((long)row * D + base) >> 3);
          short8_t o, r;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float d_ = ln_bwd_t2_dx<HASDE>(dyg[p * 8 + j], xh[p * 8 + j], s1,
                                           s2, rstd, ve[j]);
            o[j] = f32_to_bf16(d_);
            r[j] = drop_grad(d_, (keep >> j) & 1, dr.scale);
          }
          *(short8_t*)(dx + (long)row * D + base) = o;
          *(short8_t*)(dres + (long)row * D + base) = r;
        };
        emit(rowA, dygA, xhA, veA[p], rstdA, s1A, s2A);
        if (actB) emit(rowA + 1, dygB, xhB, veB[p], rstdB, s1B, s2B);
        continue;
      }
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
// DROP: as in ln_bwd_t2, a second output dres.
template <int MAXP, bool DRES, bool DROP>
__global__ void __launch_bounds__(BLOCK)
ln_bwd_g(const short* __restrict__ dy, const short* __restrict__ x,
         const short* __restrict__ gamma, const float* __restrict__ mean_in,
         const float* __restrict__ rstd_in,
         const short* __restrict__ ds_extra,  // optional += into dx
         short* __restrict__ dx, float* __restrict__ ws, int N, int D,
         short* __restrict__ dres, LnDrop dr) {
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
      short8_t o, r;
      unsigned keep = 0;
      if (DROP) keep = drop_keep8(dr, ((long)row * D + base) >> 3);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float h = (bf16_to_f32(vx[p][j]) - mean) * rstd;
        float g = bf16_to_f32(vd[p][j]) * bf16_to_f32(vg[p][j]);
        float d_;
        if (DROP) {
          // the sibling's fusing (every product into the add after it),
          // spelled out: see mul_rn
          const float t = __builtin_fmaf(
              -h, s2, __builtin_fmaf(bf16_to_f32(vd[p][j]),
                                     bf16_to_f32(vg[p][j]), -s1));
          d_ = der ? __builtin_fmaf(rstd, t, bf16_to_f32(ev[j])) : rstd * t;
          r[j] = drop_grad(d_, (keep >> j) & 1, dr.scale);
        } else {
          d_ = rstd * (g - s1 - h * s2);
          if (der) d_ += bf16_to_f32(ev[j]);
        }
        o[j] = f32_to_bf16(d_);
        // the sum of what is STORED: round first, then accumulate
        if (DRES) acc[NOUT - 1][p * 8 + j] += bf16_to_f32(o[j]);
      }
      *(short8_t*)(dxr + base) = o;
      if (DROP) *(short8_t*)(dres + (long)row * D + base) = r;
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

// One dispatch per direction, shared by the plain and the dropout launchers:
// DROP only selects the instantiation, so both take the same kernel variant
// and the same grid at every width.
// MX (never with DROP) selects the MX-output kernel of the same variant:
// y = q, mean = the scale bytes, rstd = nullptr (the table at LnMxOut above).
template <bool DROP, bool MX = false>
static hipError_t ln_fwd_dispatch(const void* x, const void* res,
                                  const void* gamma, const void* beta, void* y,
                                  void* s_out, void* mean, void* rstd, int N,
                                  int D, float eps, LnDrop dr,
                                  hipStream_t stream) {
  static_assert(!(DROP && MX), "no dropout in the MX output mode");
  const int grid = ln_row_blocks(N, LN_FWD_MAX_GRID);
#define LNF_ARGS                                                              \
  (const short*)x, (const short*)res, (const short*)gamma,                    \
      (const short*)beta, (short*)y, (short*)s_out, (float*)mean,             \
      (float*)rstd, N, D, eps, dr
#define LNF_T(P)                                                              \
  do {                                                                        \
    if constexpr (MX) {                                                       \
      if (res) {                                                              \
        ln_fwd_t<P, true, false, true><<<grid, BLOCK, 0, stream>>>(LNF_ARGS);  \
      } else {                                                                \
        ln_fwd_t<P, false, false, true><<<grid, BLOCK, 0, stream>>>(LNF_ARGS); \
      }                                                                       \
    } else if (res) {                                                         \
      ln_fwd_t<P, true, DROP, false><<<grid, BLOCK, 0, stream>>>(LNF_ARGS);   \
    } else if constexpr (!DROP) {                                             \
      ln_fwd_t<P, false, false, false><<<grid, BLOCK, 0, stream>>>(LNF_ARGS); \
    }                                                                         \
  } while (0)
  if (D == 512) LNF_T(1);
  else if (D == 1024) LNF_T(2);
  else if (D == 2048) LNF_T(4);
  // PKTS=8 (D=4096) allocates 256 VGPRs (1 wave/SIMD) — the general kernel
  // is the better trade there
  else if constexpr (MX)
    ln_fwd_kernel<false, true><<<grid, BLOCK, 0, stream>>>(LNF_ARGS);
  else
    ln_fwd_kernel<DROP, false><<<grid, BLOCK, 0, stream>>>(LNF_ARGS);
#undef LNF_T
#undef LNF_ARGS
  return hipGetLastError();
}

// runtime A/B: TOSEM_LN_BWD=1row selects the single-row ln_bwd_t variant
// (no dropout instantiation: the dropout launcher always runs ln_bwd_t2)
static int ln_bwd_use_1row() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("TOSEM_LN_BWD");
    v = (e && strcmp(e, "1row") == 0) ? 1 : 0;
  }
  return v;
}

// DROP: n_out is 2 and dres_out the [N, D] gradient of the dropped residual;
// D <= LN_BWD_G_MAX_D.
template <bool DROP>
static hipError_t ln_bwd_dispatch(const void* dy, const void* x,
                                  const void* gamma, const void* mean,
                                  const void* rstd, const void* ds_extra,
                                  void* dx, void* ws, int n_out, int N, int D,
                                  void* dres_out, LnDrop dr,
                                  hipStream_t stream) {
  const int grid = ln_bwd_grid(N, D);
  const bool dres = n_out == 3;
  size_t shm = (size_t)D * n_out * sizeof(float);
#define LNB_ARGS                                                              \
  (const short*)dy, (const short*)x, (const short*)gamma, (const float*)mean, \
      (const float*)rstd, (const short*)ds_extra, (short*)dx, (float*)ws, N, D
#define LNB_DROP (short*)dres_out, dr
#define LNB_T1(P)                                                             \
  do {                                                                        \
    if (ds_extra && dres) {                                                   \
      ln_bwd_t<P, true, true><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);          \
    } else if (ds_extra) {                                                    \
      ln_bwd_t<P, true, false><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);         \
    } else if (dres) {                                                        \
      ln_bwd_t<P, false, true><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);         \
    } else {                                                                  \
      ln_bwd_t<P, false, false><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);        \
    }                                                                         \
  } while (0)
#define LNB_T2(P)                                                             \
  do {                                                                        \
    if (!dres && ds_extra) {                                                  \
      ln_bwd_t2<P, true, false, DROP><<<grid, BLOCK, 0, stream>>>(            \
          LNB_ARGS, LNB_DROP);                                                \
    } else if (!dres) {                                                       \
      ln_bwd_t2<P, false, false, DROP><<<grid, BLOCK, 0, stream>>>(           \
          LNB_ARGS, LNB_DROP);                                                \
    } else if constexpr (!DROP) {                                             \
      if (ds_extra) {                                                         \
        ln_bwd_t2<P, true, true, false><<<grid, BLOCK, 0, stream>>>(          \
            LNB_ARGS, LNB_DROP);                                              \
      } else {                                                                \
        ln_bwd_t2<P, false, true, false><<<grid, BLOCK, 0, stream>>>(         \
            LNB_ARGS, LNB_DROP);                                              \
      }                                                                       \
    }                                                                         \
  } while (0)
#define LNB_T(P)                                                              \
  do {                                                                        \
    if (!DROP && ln_bwd_use_1row()) {                                         \
      LNB_T1(P);                                                              \
    } else {                                                                  \
      LNB_T2(P);                                                              \
    }                                                                         \
  } while (0)
#define LNB_G(P)                                                              \
  do {                                                                        \
    if (!dres) {                                                              \
      ln_bwd_g<P, false, DROP><<<grid, BLOCK, shm, stream>>>(LNB_ARGS,        \
                                                             LNB_DROP);       \
    } else if constexpr (!DROP) {                                             \
      ln_bwd_g<P, true, false><<<grid, BLOCK, shm, stream>>>(LNB_ARGS,        \
                                                             LNB_DROP);       \
    }                                                                         \
  } while (0)
  if (D == 512) LNB_T(1);
  else if (D == 1024) LNB_T(2);
  else if (D <= 512) LNB_G(1);
  else if (D <= 1024) LNB_G(2);
  else if (D <= 2048) LNB_G(4);
  else if (D <= LN_BWD_G_MAX_D) LNB_G(8);
  else if constexpr (!DROP) {
    if (dres) {
      ln_bwd_wide_kernel<true><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);
    } else {
      ln_bwd_wide_kernel<false><<<grid, BLOCK, 0, stream>>>(LNB_ARGS);
    }
  }
#undef LNB_G
#undef LNB_T
#undef LNB_T2
#undef LNB_T1
#undef LNB_DROP
#undef LNB_ARGS
  return hipGetLastError();
}

// thr in [1, 65535]; the scale is formed in double and rounded once, like
// reference.dropout_threshold's
static bool ln_drop_args(unsigned long long seed, unsigned call, unsigned site,
                         unsigned thr, LnDrop* dr) {
  if (thr < 1 || thr > 65535) return false;
  *dr = LnDrop{(unsigned)seed, (unsigned)(seed >> 32), call, site, thr,
               (float)(65536.0 / (double)(65536 - thr))};
  return true;
}

extern "C" {

hipError_t ln_fwd_launch(const void* x, const void* res, const void* gamma,
                         const void* beta, void* y, void* s_out, void* mean,
                         void* rstd, int N, int D, float eps,
                         hipStream_t stream) {
  return ln_fwd_dispatch<false>(x, res, gamma, beta, y, s_out, mean, rstd, N,
                                D, eps, LnDrop{}, stream);
}

hipError_t ln_drop_fwd_launch(const void* x, const void* res,
                              const void* gamma, const void* beta, void* y,
                              void* s_out, void* mean, void* rstd, int N,
                              int D, float eps, unsigned long long seed,
                              unsigned call, unsigned site, unsigned thr,
                              hipStream_t stream) {
  LnDrop dr;
  if (!res || !s_out || !ln_drop_args(seed, call, site, thr, &dr))
    return hipErrorInvalidValue;
  return ln_fwd_dispatch<true>(x, res, gamma, beta, y, s_out, mean, rstd, N,
                               D, eps, dr, stream);
}

hipError_t ln_mx_fwd_launch(const void* x, const void* res, const void* gamma,
                            const void* beta, void* q, void* scales,
                            void* s_out, int N, int D, float eps,
                            hipStream_t stream) {
  if (D <= 0 || D % 32 || D > ln_mx_fwd_max_d() || !res != !s_out)
    return hipErrorInvalidValue;
  return ln_fwd_dispatch<false, true>(x, res, gamma, beta, q, s_out, scales,
                                      nullptr, N, D, eps, LnDrop{}, stream);
}

int ln_mx_fwd_max_d(void) { return 4096; }

// ws is [ln_bwd_ws_rows(N, D), n_out * D] f32 with n_out = 2
// ([dgamma | dbeta]) or 3 (+ [dres_sum]); every width supports both.
hipError_t ln_bwd_launch(const void* dy, const void* x, const void* gamma,
                         const void* mean, const void* rstd,
                         const void* ds_extra, void* dx, void* ws, int n_out,
                         int N, int D, hipStream_t stream) {
  if (n_out != 2 && n_out != 3) return hipErrorInvalidValue;
  return ln_bwd_dispatch<false>(dy, x, gamma, mean, rstd, ds_extra, dx, ws,
                                n_out, N, D, nullptr, LnDrop{}, stream);
}

hipError_t ln_drop_bwd_launch(const void* dy, const void* x,
                              const void* gamma, const void* mean,
                              const void* rstd, const void* ds_extra, void* dx,
                              void* dres, void* ws, int N, int D,
                              unsigned long long seed, unsigned call,
                              unsigned site, unsigned thr,
                              hipStream_t stream) {
  LnDrop dr;
  if (!dres || D > LN_BWD_G_MAX_D || !ln_drop_args(seed, call, site, thr, &dr))
    return hipErrorInvalidValue;
  return ln_bwd_dispatch<true>(dy, x, gamma, mean, rstd, ds_extra, dx, ws, 2,
                               N, D, dres, dr, stream);
}

int ln_drop_bwd_max_d(void) { return LN_BWD_G_MAX_D; }

// Workspace rows ln_bwd_launch and ln_drop_bwd_launch write: one per block
// (the waves merge through LDS), one per wave on the wide path.  Either way
// the column sum reduces them in fixed order.
int ln_bwd_ws_rows(int N, int D) {
  const int grid = ln_bwd_grid(N, D);
  return D > LN_BWD_G_MAX_D ? grid * WAVES_PER_BLOCK : grid;
}

}  // extern "C"

