// Flash attention for gfx950 (CDNA4) — bf16 I/O, f32 online softmax, MFMA
// (v_mfma_f32_32x32x16_bf16) everywhere, head_dim = 64.
//
// Never materializes the [L, L] score matrix.  Four MFMA kernels:
//   flash_fwd_kernel           O and the per-row logsumexp
//   flash_bwd_fused_kernel     dK, dV (one wave per 32-row kv block)
//   flash_dq_recompute_kernel  dQ, recomputing S/dP/dS in registers
//   flash_dq_kernel            dQ = dS @ K from a materialized dS (A/B path)
// plus fa_dot (D = rowsum(dO * O), and one flag per 32-row query tile whose
// dO is all +-0, which the two backward kernels then leave out).  The
// default backward is fa_dot + flash_bwd_fused + flash_dq_recompute.
//
// Shared structure (guide §B "fused attention prefill" adapted):
//  * swapped QK^T — compute mfma(A=K, B=Q^T) so the score column for one
//    q-row is LANE-LOCAL (16 regs + the partner lane at lane^32): softmax is
//    15 in-lane max/sum ops + one __shfl_xor(32) exchange, no LDS round trip.
//  * C-layout -> A-fragments via v_cvt_pk_bf16_f32 pairs + permlane32_swap
//    (guide T12): 8 cvt_pk + 4 swaps replace any cross-lane scatter.
//  * every staged tile (K, V, Q, dO) is [32][64] bf16 row-major in LDS with
//    the T2 XOR swizzle (byte ^= (row&7)<<4): the row-fragment ds_read_b128
//    is ~conflict-free, and the TRANSPOSED fragment of the same tile is
//    gathered with ds_read_b64_tr_b16 — no second, transposed copy.
//  * workgroup = 4 waves sharing the staged tiles.  In the q-major kernels
//    (fwd, dq, dq-recompute) each wave owns TWO 32-row q-blocks, so a
//    workgroup covers 256 q rows; in flash_bwd_fused each wave owns one
//    32-row kv block, so a workgroup covers 128 kv rows.

#include "common.h"
#include "launchers.h"
#include "philox.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned uint2_t;
typedef __attribute__((ext_vector_type(4))) unsigned uint4_t;

#define FA_DH 64
#define FA_KVB 32
#define FA_QB 32          // q rows per q-block
#define FA_WAVES 4
#define FA_BLOCK (FA_WAVES * WAVE)
#define FA_QWG (FA_WAVES * FA_QB)   // 128 rows: one 32-row block per wave
#define FA_Q2WG (2 * FA_QWG)        // 256 q rows: two q-blocks per wave

// LDS (dynamic, 16-B aligned).  One staged tile is [32][64] bf16, row
// stride 128 B, XOR-swizzled = 4096 B.  Per kernel:
//  fwd:          K tile | V tile | alpha [4 waves][64] f32 (1024 B; its
//                first words double as the tail-skip / segment-range scratch
//                before the loop) | side [32]
//  bwd_fused:    Q tile | dO tile | lse [32] f32 | ddot [32] f32
//                (segmented: + the staged tile's q segment ids [32] i32)
//  dq:           K tile
//  dq_recompute: K tile | V tile | side [32] | 16 B tail-skip scratch
// side is the staged kv tile's per-key side data, one 4-byte word per key:
// the mask bias (f32) or, segmented, the kv segment id (i32).  A slot of its
// own: the scratch words are still being read when the first tile is staged.
#define TILE_LDS_BYTES (FA_KVB * 128)
#define SIDE_LDS_BYTES (FA_KVB * 4)
#define FWD_LDS_BYTES                                                         \
  (2 * TILE_LDS_BYTES + FA_WAVES * 64 * sizeof(float) + SIDE_LDS_BYTES)
#define BWD_LDS_BYTES (2 * TILE_LDS_BYTES + 64 * sizeof(float))
#define BWD_SEG_LDS_BYTES (BWD_LDS_BYTES + 32 * sizeof(int))
#define DQ_LDS_BYTES TILE_LDS_BYTES
#define DQR_LDS_BYTES (2 * TILE_LDS_BYTES + SIDE_LDS_BYTES + 16)
// Waves per SIMD flash_dq_recompute is bounded to.  Without dropout it fits
// two with nothing to spare (256 VGPRs); with the mask's temporaries it
// spilled 56-112 B per lane under that bound, so the DROP instantiations are
// bounded to one: lower occupancy, no scratch.
#define FA_DQR_WAVES(drop) ((drop) ? 1 : 2)

// Tensor geometry: the kernels address q/k/v rows as
//   base + b*qkv_bs + h*qkv_hs + l*qkv_rs        (64 contiguous shorts)
// and o/dout rows as b*o_bs + h*o_hs + l*o_rs — so the SAME kernels run on
// the bmm-style [B, H, L, 64] layout and directly on the packed
// QKV-projection output [B, L, 3D] (k/v at base offset D/2D) with the
// attention output written straight into the [B, L, D] proj input.  The
// packed path deletes the four qkv/out repack kernels (+their backward
// merges) from the model step.
struct FaGeom {
  long qkv_bs, qkv_hs; int qkv_rs;
  long o_bs, o_hs; int o_rs;
  static FaGeom bhld(int H, int L) {        // q/k/v/o all [B, H, L, 64]
    return {(long)H * L * FA_DH, (long)L * FA_DH, FA_DH,
            (long)H * L * FA_DH, (long)L * FA_DH, FA_DH};
  }
  static FaGeom packed(int H, int L) {      // qkv [B, L, 3D], o [B, L, D]
    const int D = H * FA_DH;
    return {(long)L * 3 * D, 64L, 3 * D, (long)L * D, 64L, D};
  }
};

// ---- fragment plumbing shared by the four MFMA kernels ----------------------
// All of it encodes the 32x32x16 MFMA register layouts and the lane-grid
// law of ds_read_b64_tr_b16 pinned by scripts/tr_probe.py; a tile-layout or
// swizzle change is made here, once.

__device__ __forceinline__ int kswz(int row, int byte_off) {
  return byte_off ^ ((row & 7) << 4);
}

// C-layout row map: accumulator register r of the lane half `half` holds
// row c_row(r, half) of the 32x32 result (the lane's column is lane & 31).
__device__ __forceinline__ int c_row(int r, int half) {
  return (r & 3) + 8 * (r >> 2) + 4 * half;
}

// Tile staging: 256 threads move one [32][64] bf16 tile, 16 B each.  load()
// reads this thread's piece of the tile starting at global row `row0` (rows
// `rs` shorts apart) into a register — issued one tile ahead as the
// prefetch — and store() writes it to the swizzled LDS tile.
struct FaStager {
  int row, byte;
  __device__ __forceinline__ explicit FaStager(int tid)
      : row(tid >> 3), byte((tid & 7) * 16) {}
  __device__ __forceinline__ short8_t load(const short* base, int row0,
                                           int rs) const {
    return *(const short8_t*)(base + (long)(row0 + row) * rs + (byte >> 1));
  }
  __device__ __forceinline__ void store(short* lds, short8_t v) const {
    *(short8_t*)((char*)lds + row * 128 + kswz(row, byte)) = v;
  }
};

// Per-tile side data travels with its tile.  A kv tile's 32 mask biases or
// segment ids (a q tile's lse, ddot and segment ids in flash_bwd_fused) are
// loaded by threads 0..31 in the same slot as the tile's prefetch, sit in a
// register through the iteration and go to LDS next to st.store, between the
// loop-top barriers.  The loop body then reads them with ds_read, which
// counts on lgkmcnt: vmcnt retires in issue order, so a global load issued
// after the prefetch and used inside the body would drain the prefetch at
// its first use.  fa_side_rows fills the 16 register-row values of a lane
// half from the staged words: c_row(r, half) is four runs of four
// consecutive rows, each starting at a multiple of four, so it is four
// 16-byte reads.
template <typename T>
__device__ __forceinline__ void fa_side_rows(const T* side, int half,
                                             T (&out)[16]) {
  typedef __attribute__((ext_vector_type(4))) T vec4;
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const vec4 w = *(const vec4*)(side + 8 * gq + 4 * half);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * gq + j] = w[j];
  }
}

// Row fragment c (k = 16c .. 16c+15) of a staged tile: lane reads 8 bf16 of
// tile row `col` — the A operand of the S/dP MFMAs.
__device__ __forceinline__ short8_t tile_row_frag(const short* lds, int col,
                                                  int half, int c) {
  return *(const short8_t*)((const char*)lds + col * 128 +
                            kswz(col, (16 * c + 8 * half) * 2));
}

// C-layout f32 (reg=R, lane=C) -> bf16 A-fragments [row=C][k=R].  One step
// packs registers r0, r0+1 and r1, r1+1 and swaps lane halves; it yields
// words i and i+2 of the fragment.  permlane32_swap needs two wait states
// after a VALU write and hipcc pads only one after inline asm, hence the
// explicit s_nop 1.
__device__ __forceinline__ void cvt_pk_swap(const float (&s)[16], int r0,
                                            int r1, uint4_t& u, int i) {
  unsigned lo, hi;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2\n\ts_nop 1" : "=v"(lo)
      : "v"(s[r0]), "v"(s[r0 + 1]));
  asm("v_cvt_pk_bf16_f32 %0, %1, %2\n\ts_nop 1" : "=v"(hi)
      : "v"(s[r1]), "v"(s[r1 + 1]));
  auto sw = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
  u[i] = sw[0]; u[i + 2] = sw[1];
}

// Every kernel repacks TWO accumulators at the same point (q-blocks A and
// B, or P and dS).  Their steps alternate, so the scheduler sees two
// independent cvt -> swap chains side by side; repacking one accumulator
// wholly before the other gives a different (measured: not faster) loop
// schedule.
__device__ __forceinline__ void c_to_afrag2(const float (&sa)[16],
                                            short8_t (&fa)[2],
                                            const float (&sb)[16],
                                            short8_t (&fb)[2]) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    uint4_t ua, ub;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int r0 = c * 8 + 2 * i;
      int r1 = c * 8 + 4 + 2 * i;
      cvt_pk_swap(sa, r0, r1, ua, i);
      cvt_pk_swap(sb, r0, r1, ub, i);
    }
    fa[c] = __builtin_bit_cast(short8_t, ua);
    fb[c] = __builtin_bit_cast(short8_t, ub);
  }
}

// Transposed fragments of a staged [32][64] tile X: the B operands
// X^T[d][row] for both 32-wide d halves (t) and both 16-row k chunks (c),
// gathered with eight ds_read_b64_tr_b16 lane-grid transpose reads.
struct FaTrFrags {
  uint2_t r[8];
  __device__ __forceinline__ short8_t frag(int c, int t) const {
    uint4_t w;
    w[0] = r[c * 4 + 0 * 2 + t][0];
    w[1] = r[c * 4 + 0 * 2 + t][1];
    w[2] = r[c * 4 + 1 * 2 + t][0];
    w[3] = r[c * 4 + 1 * 2 + t][1];
    return __builtin_bit_cast(short8_t, w);
  }
};

// tr_offsets gives the lane's eight byte offsets into a tile.  They are the
// same for every staged tile and every loop iteration, so a kernel takes
// them once, up front.
struct FaTrOffsets { unsigned a[8]; };

__device__ __forceinline__ FaTrOffsets tr_offsets(int lane, int half) {
  const int row_mate = (lane >> 2) & 3;
  const int d_lane = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  FaTrOffsets o;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        int row = 16 * c + 8 * half + 4 * rr + row_mate;
        int dcol = (32 * t + d_lane) * 2;
        o.a[c * 4 + rr * 2 + t] = row * 128 + kswz(row, dcol);
      }
  return o;
}

// tr_issue adds the tile's LDS base and issues the eight reads with their
// s_waitcnt in ONE asm volatile, so the compiler can neither split the batch
// nor sink the wait.
__device__ __forceinline__ void tr_issue(const short* lds,
                                         const FaTrOffsets& o, FaTrFrags& f) {
  const unsigned base = (unsigned)(unsigned long)(char*)lds;
  unsigned a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = base + o.a[i];
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\t"
      "ds_read_b64_tr_b16 %1, %9\n\t"
      "ds_read_b64_tr_b16 %2, %10\n\t"
      "ds_read_b64_tr_b16 %3, %11\n\t"
      "ds_read_b64_tr_b16 %4, %12\n\t"
      "ds_read_b64_tr_b16 %5, %13\n\t"
      "ds_read_b64_tr_b16 %6, %14\n\t"
      "ds_read_b64_tr_b16 %7, %15\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(f.r[0]), "=&v"(f.r[1]), "=&v"(f.r[2]), "=&v"(f.r[3]),
        "=&v"(f.r[4]), "=&v"(f.r[5]), "=&v"(f.r[6]), "=&v"(f.r[7])
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]),
        "v"(a[6]), "v"(a[7])
      : "memory");
}

// The gather proper: the reads, then a scheduling fence so the MFMA chain
// that consumes the fragments is not hoisted above them.  A kernel that
// gathers two tiles back to back (flash_bwd_fused) issues the first with
// tr_issue and fences once, after the second.
__device__ __forceinline__ void tr_gather(const short* lds,
                                          const FaTrOffsets& o, FaTrFrags& f) {
  tr_issue(lds, o, f);
  __builtin_amdgcn_sched_barrier(0);
}

// Work split of the q-major kernels: workgroup -> (b*H + h, 256-row q
// chunk), wave -> q-blocks A = rows [qA, qA+32) and B = [qB, qB+32).
struct FaQBlocks { int bh, qA, qB; };

__device__ __forceinline__ FaQBlocks fa_qblocks(int L, int wid) {
  const int n_qblocks = (L + FA_Q2WG - 1) / FA_Q2WG;
  const int bid = xcd_group_remap(blockIdx.x, gridDim.x, n_qblocks);
  const int qA = (bid % n_qblocks) * FA_Q2WG + wid * FA_QB;
  return {bid / n_qblocks, qA, qA + FA_QWG};
}

// ---- folded qkv bias gradient ------------------------------------------------
// The packed backward's dqkv is the output gradient of the qkv projection,
// so that projection's bias gradient is the column sum of dqkv over all
// B * L rows.  Both backward kernels hold their 32-row output tiles in the
// (register = row, lane = column) layout, so the BIAS instantiations (the
// others are the kernels without any of this) also emit per workgroup the column sums of the bf16-rounded values it stores:
// an in-lane chain over the 16 registers, one lane ^ 32 exchange, then the
// four waves merge through LDS in fixed wave order (no atomics: the result
// is bitwise reproducible).  bias_ws is [B * ceil(L / 128), bias_ld] f32,
// bias_ld = 3 * H * 64: one row per 128-row block of a batch element, the
// q / k / v thirds side by side, 64 columns per head.  Every element is
// written by exactly one workgroup — rows past L and skipped tiles add
// exact zeros — and one colsum chain over the rows finishes the sum.
//
// The epilogues add bf16_to_f32 of every value they store into one f32 per
// lane and tile (rows in register order), so the rounding is shared with
// the store and the extra work is two VALU ops per element; fa_half_merge
// then adds the other half-wave's rows of the same column.
__device__ __forceinline__ float fa_half_merge(float s) {
  return s + __shfl_xor(s, 32, WAVE);
}

// Merge the waves' sums staged in cs[2][FA_WAVES][64] (wave 0 first) and
// write the two 64-column results: slot 0 to dst0, slot 1 to dst1 (either
// may be nullptr).  Threads 0..127; the caller has put a barrier between
// the staging writes and this.
__device__ __forceinline__ void fa_colsum_merge_store(const float* cs, int tid,
                                                      float* dst0,
                                                      float* dst1) {
  if (tid < 2 * FA_DH) {
    const int slot = tid / FA_DH, c = tid % FA_DH;
    const float* p = cs + slot * FA_WAVES * FA_DH + c;
    float s = p[0];
#pragma unroll
    for (int w = 1; w < FA_WAVES; ++w) s += p[w * FA_DH];
    float* dst = slot ? dst1 : dst0;
    if (dst) dst[c] = s;
  }
}

// Padding-tail tile skip: with the additive -1e9 padding bias, every score
// in a fully-masked kv tile sits below ~-1e8 and __expf underflows to
// exactly +0.0f, so the tile contributes NOTHING to the online softmax
// (alpha==1, rowsum+=0, O+=0) or to dQ — identical to not running it.  The
// mask is per-(batch, kv) so the last unmasked position is
// workgroup-uniform; tiles past it are skipped.  If the whole row is
// masked (last==-1) nothing is skipped, preserving the reference
// softmax-over-bias behavior for degenerate all-pad sequences.
__device__ __forceinline__ int fa_last_active_kv(const float* mrow, int L,
                                                 int tid, int* scratch) {
  if (tid == 0) *scratch = -1;
  __syncthreads();
  int loc = -1;
  for (int kv = tid; kv < L; kv += FA_BLOCK)
    if (mrow[kv] > -1.0e8f) loc = kv;
  if (loc >= 0) atomicMax(scratch, loc);
  __syncthreads();
  return *scratch;
}

// ---- segments (sequence packing) --------------------------------------------
// seg is int32 [B, L], non-decreasing along a row; position i attends to
// position j iff seg[b, i] == seg[b, j].  The padding tail of a row carries
// one id above every real id, so pads form their own trailing segment and
// no softmax row is empty.  The bias is the padding mask's: 0 inside the
// segment, -1e9 outside, so an out-of-segment probability is exactly +0.0f
// in forward (a running max left behind by an all-foreign tile is
// annihilated by alpha == 0 at the first own tile) and in both backward
// kernels.  That exact zero is what lets whole tiles be skipped.
#define FA_SEG_BIAS -1.0e9f

// Tile-range skip: ids are monotone, so the positions that matter to rows
// [r_lo, r_hi] of a workgroup form ONE contiguous range — from the first
// position of r_lo's segment to the last position of r_hi's.  Computed once
// per workgroup by a scan of the seg row (like fa_last_active_kv).  The
// result always contains [r_lo, r_hi] and lies inside [0, L): a seg row
// that breaks the monotone contract changes numbers, never addresses.
struct FaRange { int lo, hi; };

__device__ __forceinline__ FaRange fa_seg_range(const int* srow, int L,
                                                int r_lo, int r_hi, int tid,
                                                int* scratch) {
  const int s_first = srow[r_lo], s_last = srow[r_hi];
  if (tid == 0) { scratch[0] = r_lo; scratch[1] = r_hi; }
  __syncthreads();
  int lo = r_lo, hi = r_hi;
  for (int j = tid; j < L; j += FA_BLOCK) {
    const int s = srow[j];
    if (s == s_first) lo = min(lo, j);
    if (s == s_last) hi = max(hi, j);
  }
  atomicMin(&scratch[0], lo);
  atomicMax(&scratch[1], hi);
  __syncthreads();
  return {scratch[0], scratch[1]};
}

// Inside the range a wave still meets tiles that hold none of its own rows'
// segments (a 256-token row of ~36-token examples is mostly such tiles).
// Every probability of such a tile is +0.0f for this wave, so its MFMA and
// softmax work is skipped; the staging and the barriers are not.  r is one
// id per register row, a and b the lane's two ids (pass a twice for one).
__device__ __forceinline__ bool fa_seg_tile_live(const int (&r)[16], int a,
                                                 int b) {
  bool hit = false;
#pragma unroll
  for (int i = 0; i < 16; ++i) hit |= (r[i] == a) | (r[i] == b);
  return __builtin_amdgcn_ballot_w64(hit) != 0;
}

// ---- dead query tiles --------------------------------------------------------
// dead is uint8 [B, H, L / 32] from fa_dot (nullptr = skip nothing): 1 marks
// a 32-row query tile whose dO block is all +-0.  Such a tile adds exact
// zeros to dK and dV and its own dQ rows are zero, so both backward kernels
// leave it out.  The flags are data the previous kernel wrote, the same for
// every wave of a workgroup, so every branch on them is workgroup-uniform.
//
// fa_live_window: bit i = tile (t0 + i) exists and is live, for the 64 tiles
// from t0 — one byte load per lane and a ballot, so the result is scalar.
__device__ __forceinline__ unsigned long long fa_live_window(
    const unsigned char* dead_bh, int t0, int n_t, int lane) {
  const int t = t0 + lane;
  bool lv = t < n_t;
  if (lv && dead_bh) lv = dead_bh[t] == 0;
  return __builtin_amdgcn_ballot_w64(lv);
}

// Zero rows [q0, min(q0 + 32, L)) of a [*, 64]-column bf16 tile, rows rs
// shorts apart: one wave, 16 B per lane, eight rows per store.
__device__ __forceinline__ void fa_store_zero_tile(short* base, int rs, int q0,
                                                   int L, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = q0 + 8 * i + (lane >> 3);
    if (row < L)
      *(short8_t*)(base + (long)row * rs + (lane & 7) * 8) = (short8_t)(0);
  }
}

// Scalar scan over the windows: first live tile in [qt, n_q), or n_q.
struct FaLiveScan {
  const unsigned char* dead_bh;
  int n_t, lane, win;
  unsigned long long bits;
  __device__ __forceinline__ FaLiveScan(const unsigned char* d, int n_t_,
                                        int lane_)
      : dead_bh(d), n_t(n_t_), lane(lane_), win(-1), bits(0) {}
  // Window 0 up front, so the flag load is in flight with whatever the
  // kernel loads first instead of ahead of its first tile.
  __device__ __forceinline__ void preload() {
    if (dead_bh) { win = 0; bits = fa_live_window(dead_bh, 0, n_t, lane); }
  }
  __device__ __forceinline__ int next(int qt, int n_q) {
    if (!dead_bh) return qt;
    while (qt < n_q) {
      if ((qt >> 6) != win) {
        win = qt >> 6;
        bits = fa_live_window(dead_bh, win << 6, n_t, lane);
      }
      const unsigned long long m = bits >> (qt & 63);
      if (m) return min(qt + (int)__builtin_ctzll(m), n_q);
      qt = (win + 1) << 6;
    }
    return n_q;
  }
};

// ---- attention-probability dropout -------------------------------------------
// The mask is philox.h's: one Philox call per 4 x 4 block of P.  A lane's 16
// score registers are four groups of four consecutive rows (c_row) and its
// column is lane & 31, so register group g of the four lanes of a quad
// (lanes 4i .. 4i+3) lies in ONE block, and a 32 x 32 tile costs the quad
// four calls, one per group.  Each lane runs one of them — lane & 3 = g runs
// group g's — and the words travel through quad-broadcast DPP moves.  Every
// lane of the wave must be active at the call: the kernels only branch
// wave-uniformly around it.
//
// Both functions return the keep bits of the lane's 16 registers, bit r =
// register r, for the two layouts the kernels hold scores in.
//
// FA_DROP_QUAD_SHARE=0 builds the A/B variant in which every lane runs all
// four calls itself and nothing crosses lanes: four times the integer
// multiplies, no DPP moves.  Same bits; docs/PERF.md has both timings.
#ifndef FA_DROP_QUAD_SHARE
#define FA_DROP_QUAD_SHARE 1
#endif

template <int G>
__device__ __forceinline__ unsigned fa_quad_bcast(unsigned v) {
  return (unsigned)__builtin_amdgcn_mov_dpp((int)v, G * 0x55, 0xf, 0xf, true);
}

// (register = kv, lane = q), forward and dq-recompute.  The lane's q is
// fixed, so its bits are ONE word (q & 3 = lane & 3) of each group's call, a
// byte per register.
template <int G>
__device__ __forceinline__ unsigned fa_drop_group_kvreg(const unsigned (&w)[4],
                                                        int i, unsigned thr) {
  const unsigned t0 = fa_quad_bcast<G>(w[0]), t1 = fa_quad_bcast<G>(w[1]);
  const unsigned t2 = fa_quad_bcast<G>(w[2]), t3 = fa_quad_bcast<G>(w[3]);
  const unsigned word = i == 0 ? t0 : i == 1 ? t1 : i == 2 ? t2 : t3;
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    m |= (((word >> (8 * j)) & 0xffu) >= thr ? 1u : 0u) << (4 * G + j);
  return m;
}

// rowblk: index of block (q / 4, 0) of this lane's (b, h, q);
// kblk0 = kv0 / 4 + half, the block column of register group 0.
__device__ __forceinline__ unsigned fa_drop_keep16_kvreg(
    const FaDrop& dr, unsigned long long rowblk, int kblk0, int lane) {
  const int i = lane & 3;
  unsigned w[4];
#if FA_DROP_QUAD_SHARE
  fa_drop_block(dr, rowblk + (unsigned)(kblk0 + 2 * i), w);
  return fa_drop_group_kvreg<0>(w, i, dr.thr) |
         fa_drop_group_kvreg<1>(w, i, dr.thr) |
         fa_drop_group_kvreg<2>(w, i, dr.thr) |
         fa_drop_group_kvreg<3>(w, i, dr.thr);
#else
  unsigned m = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    fa_drop_block(dr, rowblk + (unsigned)(kblk0 + 2 * g), w);
    const unsigned word = i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      m |= (((word >> (8 * j)) & 0xffu) >= dr.thr ? 1u : 0u) << (4 * g + j);
  }
  return m;
#endif
}

// (register = q, lane = kv), flash_bwd_fused.  The lane's kv is fixed: its
// bits are ONE byte (k & 3 = lane & 3) of every word of each group's call.
template <int G>
__device__ __forceinline__ unsigned fa_drop_group_qreg(const unsigned (&w)[4],
                                                       int sh, unsigned thr) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    m |= (((fa_quad_bcast<G>(w[j]) >> sh) & 0xffu) >= thr ? 1u : 0u)
         << (4 * G + j);
  return m;
}

// colblk: index of block (0, kv / 4) of this lane's (b, h, kv); nb = L / 4;
// qblk0 = q0 / 4 + half, the block row of register group 0.
__device__ __forceinline__ unsigned fa_drop_keep16_qreg(
    const FaDrop& dr, unsigned long long colblk, unsigned nb, int qblk0,
    int lane) {
  const int i = lane & 3;
  unsigned w[4];
#if FA_DROP_QUAD_SHARE
  fa_drop_block(dr, colblk + (unsigned long long)(qblk0 + 2 * i) * nb, w);
  return fa_drop_group_qreg<0>(w, 8 * i, dr.thr) |
         fa_drop_group_qreg<1>(w, 8 * i, dr.thr) |
         fa_drop_group_qreg<2>(w, 8 * i, dr.thr) |
         fa_drop_group_qreg<3>(w, 8 * i, dr.thr);
#else
  unsigned m = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    fa_drop_block(dr, colblk + (unsigned long long)(qblk0 + 2 * g) * nb, w);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      m |= (((w[j] >> (8 * i)) & 0xffu) >= dr.thr ? 1u : 0u) << (4 * g + j);
  }
  return m;
#endif
}

// DROP: dropout on the probabilities.  The running max, the row sum and lse
// stay those of the UNDROPPED softmax; the dropped entries of P are zeroed
// just before the PV product and the scale rides on the epilogue's 1 / l.
template <bool SEG, bool DROP>
__global__ void __launch_bounds__(FA_BLOCK, 2)
flash_fwd_kernel(const short* __restrict__ q, const short* __restrict__ k,
                 const short* __restrict__ v, const float* __restrict__ mask,
                 const int* __restrict__ seg,
                 short* __restrict__ o, float* __restrict__ lse,
                 int B, int H, int L, float scale, FaGeom g, FaDrop dr) {
  // Each wave processes TWO independent 32-row q-blocks against the shared
  // K/V tile: the second block's MFMAs overlap the first block's serial
  // softmax chain (ILP within the wave).  2 waves/SIMD by registers.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* k_lds = (short*)smem;
  short* v_lds = (short*)(smem + TILE_LDS_BYTES);
  float* alpha_lds = (float*)(smem + 2 * TILE_LDS_BYTES);
  float* mb_lds = alpha_lds + FA_WAVES * 64;   // side [32]: bias or seg id
  int* sk_lds = (int*)mb_lds;

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int col = lane & 31;
  const int half = lane >> 5;
  const FaTrOffsets tro = tr_offsets(lane, half);

  const FaQBlocks qb = fa_qblocks(L, wid);
  const int b = qb.bh / H;
  const int h = qb.bh % H;
  const long qkv_off = (long)b * g.qkv_bs + (long)h * g.qkv_hs;
  const long o_off = (long)b * g.o_bs + (long)h * g.o_hs;
  const int my_qA = qb.qA + col;
  const int my_qB = qb.qB + col;
  const bool validA = my_qA < L;
  const bool validB = my_qB < L;
  const float* mrow = (!SEG && mask) ? mask + (long)b * L : nullptr;
  const int* srow = SEG ? seg + (long)b * L : nullptr;
  // q segment ids: one lane-local scalar per q-block
  int sqA = 0, sqB = 0;
  if constexpr (SEG) {
    sqA = srow[validA ? my_qA : L - 1];
    sqB = srow[validB ? my_qB : L - 1];
  }

  short8_t qfA[4], qfB[4];
  {
    const short* qrA = q + qkv_off + (long)(validA ? my_qA : L - 1) * g.qkv_rs;
    const short* qrB = q + qkv_off + (long)(validB ? my_qB : L - 1) * g.qkv_rs;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      qfA[c] = *(const short8_t*)(qrA + c * 16 + half * 8);
      qfB[c] = *(const short8_t*)(qrB + c * 16 + half * 8);
    }
  }

  f32x16 oA[2], oB[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { oA[t] = (f32x16)(0.f); oB[t] = (f32x16)(0.f); }
  float mA = -3.0e38f, lA = 0.f, mB = -3.0e38f, lB = 0.f;
  // DROP: the mask blocks of this lane's two q rows, block column 0
  unsigned long long dblkA = 0, dblkB = 0;
  if constexpr (DROP) {
    const unsigned long long nb = (unsigned)L / 4;
    dblkA = ((unsigned long long)qb.bh * nb + (unsigned)(my_qA >> 2)) * nb;
    dblkB = ((unsigned long long)qb.bh * nb + (unsigned)(my_qB >> 2)) * nb;
  }

  const int n_kv = L / FA_KVB;
  int kt_begin = 0;
  int n_kv_eff = n_kv;
  if (mrow) {
    int last = fa_last_active_kv(mrow, L, tid, (int*)alpha_lds);
    if (last >= 0) n_kv_eff = min(n_kv, last / FA_KVB + 1);
  }
  if constexpr (SEG) {
    const int q_lo = qb.qA - wid * FA_QB;        // the workgroup's first q row
    const FaRange kr = fa_seg_range(srow, L, q_lo, min(q_lo + FA_Q2WG, L) - 1,
                                    tid, (int*)alpha_lds);
    kt_begin = kr.lo / FA_KVB;
    n_kv_eff = kr.hi / FA_KVB + 1;
  }
  const FaStager st(tid);
  short8_t kv8 = st.load(k + qkv_off, kt_begin * FA_KVB, g.qkv_rs);
  short8_t vv8 = st.load(v + qkv_off, kt_begin * FA_KVB, g.qkv_rs);
  // the tile's side word (fa_side_rows), threads 0..31
  const bool side_ld = (SEG || mrow) && tid < FA_KVB;
  float mb_n = 0.f;
  int sk_n = 0;
  if (side_ld) {
    if constexpr (SEG) sk_n = srow[kt_begin * FA_KVB + tid];
    else mb_n = mrow[kt_begin * FA_KVB + tid];
  }
  for (int kt = kt_begin; kt < n_kv_eff; ++kt) {
    const int kv0 = kt * FA_KVB;
    __syncthreads();
    st.store(k_lds, kv8);
    st.store(v_lds, vv8);
    if (side_ld) {
      if constexpr (SEG) sk_lds[tid] = sk_n;
      else mb_lds[tid] = mb_n;
    }
    __syncthreads();
    if (kt + 1 < n_kv_eff) {
      kv8 = st.load(k + qkv_off, kv0 + FA_KVB, g.qkv_rs);
      vv8 = st.load(v + qkv_off, kv0 + FA_KVB, g.qkv_rs);
      if (side_ld) {
        if constexpr (SEG) sk_n = srow[kv0 + FA_KVB + tid];
        else mb_n = mrow[kv0 + FA_KVB + tid];
      }
    }

    // the staged tile's mask biases by register row, read above the QK
    // chain so that the reads are not on the serial path between the mfma
    // results and the exp chain.  The kv segment ids take the bias's place.
    float mb_r[16];
    int sk_r[16];
    if constexpr (SEG) {
      fa_side_rows(sk_lds, half, sk_r);
    } else if (mrow) {
      fa_side_rows(mb_lds, half, mb_r);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) mb_r[r] = 0.f;
    }
    if constexpr (SEG) {
      if (!fa_seg_tile_live(sk_r, sqA, sqB)) continue;
    }

    // ---- QK^T for BOTH q-blocks (8 back-to-back MFMAs) ----
    f32x16 sA = (f32x16)(0.f), sB = (f32x16)(0.f);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      short8_t kf = tile_row_frag(k_lds, col, half, c);
      sA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfA[c], sA, 0, 0, 0);
      sB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfB[c], sB, 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- online softmax, both blocks (independent chains -> ILP) ----
    float svA[16], svB[16];
    float tmaxA = -3.0e38f, tmaxB = -3.0e38f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float mbA, mbB;
      if constexpr (SEG) {
        mbA = sk_r[r] == sqA ? 0.f : FA_SEG_BIAS;
        mbB = sk_r[r] == sqB ? 0.f : FA_SEG_BIAS;
      } else {
        mbA = mbB = mb_r[r];
      }
      float xA = sA[r] * scale + mbA;
      float xB = sB[r] * scale + mbB;
      svA[r] = xA; svB[r] = xB;
      tmaxA = fmaxf(tmaxA, xA);
      tmaxB = fmaxf(tmaxB, xB);
    }
    tmaxA = fmaxf(tmaxA, __shfl_xor(tmaxA, 32, WAVE));
    tmaxB = fmaxf(tmaxB, __shfl_xor(tmaxB, 32, WAVE));
    float mnA = fmaxf(mA, tmaxA), mnB = fmaxf(mB, tmaxB);
    float aA = __expf(mA - mnA), aB = __expf(mB - mnB);
    float rsA = 0.f, rsB = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      svA[r] = __expf(svA[r] - mnA);
      svB[r] = __expf(svB[r] - mnB);
      rsA += svA[r];
      rsB += svB[r];
    }
    rsA += __shfl_xor(rsA, 32, WAVE);
    rsB += __shfl_xor(rsB, 32, WAVE);
    lA = lA * aA + rsA; mA = mnA;
    lB = lB * aB + rsB; mB = mnB;

    // O rescale: alpha for q-row r lives in lane r, but the O accumulators
    // hold q rows by REGISTER, so each lane needs 16 other lanes' alphas.
    // They are broadcast through the wave's own alpha_lds slice, and the
    // whole rescale is skipped wave-uniformly when no row's running max
    // moved this tile (aA==aB==1 exactly; common once the max stabilizes
    // a few tiles in).  Wave-local state only, so the uniform skip is
    // race-free.
    if (__builtin_amdgcn_ballot_w64(aA != 1.f || aB != 1.f)) {
      // LDS broadcast beat a per-register __shfl chain here (382 vs
      // ~368 us measured): 32 dependent v_readlane+mul pairs serialize
      // worse than the batched ds_read round-trip
      alpha_lds[wid * 64 + col] = aA;
      alpha_lds[wid * 64 + 32 + col] = aB;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int qrow = c_row(r, half);
          oA[t][r] *= alpha_lds[wid * 64 + qrow];
          oB[t][r] *= alpha_lds[wid * 64 + 32 + qrow];
        }
      }
    }

    // ---- dropout: the row statistics above saw every probability ----
    if constexpr (DROP) {
      const unsigned keepA =
          fa_drop_keep16_kvreg(dr, dblkA, kv0 / 4 + half, lane);
      const unsigned keepB =
          fa_drop_keep16_kvreg(dr, dblkB, kv0 / 4 + half, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!((keepA >> r) & 1u)) svA[r] = 0.f;
        if (!((keepB >> r) & 1u)) svB[r] = 0.f;
      }
    }

    // ---- P -> bf16 A-fragments, both blocks ----
    short8_t pfA[2], pfB[2];
    c_to_afrag2(svA, pfA, svB, pfB);

    // ---- PV for both blocks from tr_b16-gathered V^T fragments ----
    FaTrFrags vT;
    tr_gather(v_lds, tro, vT);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        short8_t vf = vT.frag(c, t);
        oA[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfA[c], vf, oA[t],
                                                        0, 0, 0);
        oB[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pfB[c], vf, oB[t],
                                                        0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue: both blocks ----
  if (lse != nullptr && half == 0) {
    if (validA) lse[(long)qb.bh * L + my_qA] = mA + __logf(lA);
    if (validB) lse[(long)qb.bh * L + my_qB] = mB + __logf(lB);
  }
  const float one = DROP ? dr.scale : 1.0f;
  const float invA = one / lA, invB = one / lB;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int rloc = c_row(r, half);
    float iA = __shfl(invA, rloc, WAVE);
    float iB = __shfl(invB, rloc, WAVE);
    int qA = qb.qA + rloc, qB = qb.qB + rloc;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (qA < L)
        o[o_off + (long)qA * g.o_rs + 32 * t + col] =
            f32_to_bf16(oA[t][r] * iA);
      if (qB < L)
        o[o_off + (long)qB * g.o_rs + 32 * t + col] =
            f32_to_bf16(oB[t][r] * iB);
    }
  }
}

// Grid of a kernel whose workgroup owns `rows_per_wg` rows of one (b, h).
static int fa_row_blocks(int B, int L, int rows_per_wg) {
  return B * ((L + rows_per_wg - 1) / rows_per_wg);
}
static dim3 fa_grid(int B, int H, int L, int rows_per_wg) {
  return dim3(H * fa_row_blocks(B, L, rows_per_wg));
}

// Rows of the packed backward's bias_ws: one per FA_QWG-row block of a batch
// element, i.e. the fused backward's grid over one head.
extern "C" int flash_bias_ws_rows(int B, int L) {
  return fa_row_blocks(B, L, FA_QWG);
}

// Every launcher below takes an optional seg (int32 [B, L], nullptr = none)
// and picks the segmented instantiation when it is given; mask and seg are
// mutually exclusive (the bindings enforce it).
static void fa_fwd_dispatch(const short* q, const short* k, const short* v,
                            const void* mask, const void* seg, void* o,
                            void* lse, int B, int H, int L, float scale,
                            FaGeom g, FaDrop dr, hipStream_t stream) {
  const dim3 grid = fa_grid(B, H, L, FA_Q2WG);
#define FA_FWD_SEG_ARGS                                                       \
  q, k, v, nullptr, (const int*)seg, (short*)o, (float*)lse, B, H, L, scale,  \
      g, dr
#define FA_FWD_ARGS                                                           \
  q, k, v, (const float*)mask, nullptr, (short*)o, (float*)lse, B, H, L,      \
      scale, g, dr
  if (seg && dr.thr)
    flash_fwd_kernel<true, true><<<grid, FA_BLOCK, FWD_LDS_BYTES, stream>>>(
        FA_FWD_SEG_ARGS);
  else if (seg)
    flash_fwd_kernel<true, false><<<grid, FA_BLOCK, FWD_LDS_BYTES, stream>>>(
        FA_FWD_SEG_ARGS);
  else if (dr.thr)
    flash_fwd_kernel<false, true><<<grid, FA_BLOCK, FWD_LDS_BYTES, stream>>>(
        FA_FWD_ARGS);
  else
    flash_fwd_kernel<false, false><<<grid, FA_BLOCK, FWD_LDS_BYTES, stream>>>(
        FA_FWD_ARGS);
#undef FA_FWD_ARGS
#undef FA_FWD_SEG_ARGS
}

// The launchers' dropout words (philox.h): thr = 0 is no dropout, anything
// above 255 is refused.
static bool fa_drop_ok(unsigned thr) { return thr <= 255u; }

extern "C" hipError_t flash_fwd_launch(const void* q, const void* k,
                                       const void* v, const void* mask,
                                       const void* seg, void* o, void* lse,
                                       int B, int H, int L, float scale,
                                       unsigned long long drop_seed,
                                       unsigned drop_call, unsigned drop_site,
                                       unsigned drop_thr,
                                       hipStream_t stream) {
  if (!fa_drop_ok(drop_thr)) return hipErrorInvalidValue;
  fa_fwd_dispatch((const short*)q, (const short*)k, (const short*)v, mask,
                  seg, o, lse, B, H, L, scale, FaGeom::bhld(H, L),
                  fa_drop_make(drop_seed, drop_call, drop_site, drop_thr),
                  stream);
  return hipGetLastError();
}

// qkv: [B, L, 3D] packed projection output (D = H*64); o: [B, L, D]
extern "C" hipError_t flash_fwd_packed_launch(const void* qkv,
                                              const void* mask,
                                              const void* seg, void* o,
                                              void* lse, int B, int H, int L,
                                              float scale,
                                              unsigned long long drop_seed,
                                              unsigned drop_call,
                                              unsigned drop_site,
                                              unsigned drop_thr,
                                              hipStream_t stream) {
  if (!fa_drop_ok(drop_thr)) return hipErrorInvalidValue;
  const int D = H * FA_DH;
  fa_fwd_dispatch((const short*)qkv, (const short*)qkv + D,
                  (const short*)qkv + 2 * D, mask, seg, o, lse, B, H, L,
                  scale, FaGeom::packed(H, L),
                  fa_drop_make(drop_seed, drop_call, drop_site, drop_thr),
                  stream);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Flash backward, dK/dV half: ONE kernel recomputes P and dS and
// accumulates dK and dV in registers.
//
//   P[q, kv]  = exp(scale * S + mask_bias[kv] - lse[q])
//   dP[q, kv] = dO @ V^T
//   dS[q, kv] = scale * P * (dP - D[q]),  D = rowsum(dO * O)
//   dV[kv, d] = sum_q P[q, kv]  * dO[q, d]   (register accumulators)
//   dK[kv, d] = sum_q dS[q, kv] * Q[q, d]    (register accumulators)
//
// Each wave owns one 32-row KV block: K/V fragments and the dV/dK f32
// accumulators stay in registers for the whole kernel; the workgroup's 4
// waves share LDS-staged Q/dO tiles (32 q rows per tile).  Per tile the
// wave computes S and dP in the (reg=q, lane=kv) orientation — so lse/ddot
// index by register and the mask bias is one scalar per lane — then
// repacks P and dS into A-fragments [row=kv][k=q] and feeds two MFMA
// accumulation chains against dO^T / Q^T fragments gathered from the
// already-staged tiles.  Keeping the whole contraction in one kernel avoids
// the [512,512,64]-shaped batched bmms, which ran at ~107 TF in hipBLASLt
// (see profiles/).
//
// dQ is not produced here: by default it comes from
// flash_dq_recompute_kernel.  With ds != nullptr the kernel additionally
// writes dS in the natural [B, H, L_q, L_kv] layout for flash_dq_kernel
// (the A/B path kept for comparison and tests).
//
// Mirrors reference capability only in spirit: the reference ships no
// attention kernels (data-only replication package).

//
// Segmented (SEG): the kv segment id is one scalar per lane, the q ids of
// the staged tile go through LDS next to lse/ddot, and only the q tiles
// inside the mirrored fa_seg_range of the workgroup's 128 kv rows are
// visited.  SEG excludes mask and the dS output.

//
// Dropout (DROP, never with BIAS or the dS output): with keep the forward's
// mask and Pd = keep * drop_scale * P the forward computed O = Pd V, so
//   dV = Pd^T dO,   dS = scale * P * (keep * drop_scale * dP - D)
// with D = rowsum(dO * O) unchanged (O is the dropped output).  keep * P goes
// into the dV chain and drop_scale onto the accumulator in the epilogue, the
// mirror of the forward's rounding points.

template <bool SEG, bool BIAS, bool DROP>
__global__ void __launch_bounds__(FA_BLOCK, 2)
flash_bwd_fused_kernel(const short* __restrict__ q, const short* __restrict__ k,
                       const short* __restrict__ v,
                       const short* __restrict__ dout,
                       const float* __restrict__ mask,
                       const int* __restrict__ seg,
                       const float* __restrict__ lse,
                       const float* __restrict__ ddot,
                       const unsigned char* __restrict__ dead,
                       short* __restrict__ ds, short* __restrict__ dk,
                       short* __restrict__ dv,
                       int B, int H, int L, float scale, FaGeom g,
                       float* __restrict__ bias_ws, int bias_ld, FaDrop dr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* q_lds = (short*)smem;
  short* do_lds = (short*)(smem + TILE_LDS_BYTES);
  float* lse_lds = (float*)(smem + 2 * TILE_LDS_BYTES);  // [32]
  float* dd_lds = lse_lds + 32;                          // [32]
  int* seg_lds = (int*)(dd_lds + 32);                    // [32], SEG only

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int col = lane & 31;
  const int half = lane >> 5;
  const FaTrOffsets tro = tr_offsets(lane, half);

  const int n_kvblocks = (L + FA_QWG - 1) / FA_QWG;   // 128 kv rows per WG
  int bid = xcd_group_remap(blockIdx.x, gridDim.x, n_kvblocks);
  int bh = bid / n_kvblocks;
  int kb = bid % n_kvblocks;
  const int b = bh / H;
  const int h = bh % H;
  const long qkv_off = (long)b * g.qkv_bs + (long)h * g.qkv_hs;
  const long o_off = (long)b * g.o_bs + (long)h * g.o_hs;
  const long bh_sq = (long)bh * L * L;
  const int kv_base = kb * FA_QWG + wid * FA_KVB;     // this wave's 32 kv rows
  const int my_kv = kv_base + col;
  const bool kv_valid = my_kv < L;                    // L%32==0: whole block
  const float* mrow = (!SEG && mask) ? mask + (long)b * L : nullptr;
  const float mb = mrow ? mrow[min(my_kv, L - 1)] : 0.f;
  const int* srow = SEG ? seg + (long)b * L : nullptr;
  int sk = 0;                                         // kv segment id (lane)
  if constexpr (SEG) sk = srow[min(my_kv, L - 1)];
  // DROP: the mask block of this lane's kv column, block row 0
  const unsigned drop_nb = (unsigned)L / 4;
  unsigned long long dblk = 0;
  if constexpr (DROP)
    dblk = (unsigned long long)bh * drop_nb * drop_nb +
           (unsigned)(min(my_kv, L - 1) >> 2);

  // Early-out: if every kv row this workgroup owns is padding
  // (bias <= -1e8) and the sequence has at least one real token, P and dS
  // are exactly +0.0f for every q — dK/dV are zero and the whole q loop is
  // skipped (the epilogue writes the zero accumulators).  Requires
  // ds == nullptr (the default path) so no dS tile is left unwritten; the
  // mrow[0] guard keeps degenerate all-pad sequences on the reference
  // softmax-over-bias behavior.  skip is workgroup-uniform (the flag is a
  // barrier-ordered workgroup reduction), so branching around the
  // barriered q loop is safe.
  // Dead query tiles (all-zero dO) are neither loaded nor staged: the q loop
  // steps from live tile to live tile and the prefetch targets the next
  // live one.  Never with ds: the A/B path must write every dS tile.
  FaLiveScan live(ds == nullptr && dead ? dead + (long)bh * (L / 32) : nullptr,
                  L / 32, lane);
  live.preload();

  bool skip_tile = false;
  bool wave_skip = false;
  if (mrow && ds == nullptr) {
    int* any_lds = (int*)lse_lds;
    if (tid == 0) *any_lds = 0;
    __syncthreads();
    if (kv_valid && mb > -1.0e8f) *any_lds = 1;
    __syncthreads();
    skip_tile = (*any_lds == 0) && (mrow[0] > -1.0e8f);
    __syncthreads();
    // Finer grain: a wave whose OWN 32 kv rows are all padding still has
    // to stage q/dO tiles and hit the barriers with the other waves, but
    // its S/dP MFMA chains, softmax/dS math and dK/dV accumulation are
    // exact zeros — skip them (wave-uniform ballot, no barriers inside
    // the skipped region).
    wave_skip = !skip_tile && (mrow[0] > -1.0e8f) &&
        __builtin_amdgcn_ballot_w64(kv_valid && mb > -1.0e8f) == 0;
  }

  // K and V fragments for this wave's kv block (resident all kernel)
  short8_t kf[4], vf[4];
  if (!skip_tile) {
    const short* kr = k + qkv_off + (long)(kv_valid ? my_kv : L - 1) * g.qkv_rs;
    const short* vr = v + qkv_off + (long)(kv_valid ? my_kv : L - 1) * g.qkv_rs;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      kf[c] = *(const short8_t*)(kr + c * 16 + half * 8);
      vf[c] = *(const short8_t*)(vr + c * 16 + half * 8);
    }
  }
  f32x16 dv_acc[2], dk_acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    dv_acc[t] = (f32x16)(0.f);
    dk_acc[t] = (f32x16)(0.f);
  }
  if (!skip_tile) {
  int qt_begin = 0;
  int n_q = L / 32;
  if constexpr (SEG) {
    const int kv_lo = kb * FA_QWG;                    // the workgroup's kv rows
    const FaRange qr = fa_seg_range(srow, L, kv_lo, min(kv_lo + FA_QWG, L) - 1,
                                    tid, (int*)lse_lds);
    qt_begin = qr.lo / 32;
    n_q = qr.hi / 32 + 1;
  }
  const FaStager st(tid);
  int qt = live.next(qt_begin, n_q), qt_next;
  short8_t qv8, dv8;
  // the q tile's side words (fa_side_rows): lse, ddot and, segmented, the q
  // segment id of row tid, threads 0..31; they follow the live-tile scan
  // with the tile they belong to
  const bool side_ld = tid < 32;
  float lse_n = 0.f, dd_n = 0.f;
  int sq_n = 0;
  if (qt < n_q) {
    qv8 = st.load(q + qkv_off, qt * 32, g.qkv_rs);
    dv8 = st.load(dout + o_off, qt * 32, g.o_rs);
    if (side_ld) {
      lse_n = lse[(long)bh * L + qt * 32 + tid];
      dd_n = ddot[(long)bh * L + qt * 32 + tid];
      if constexpr (SEG) sq_n = srow[qt * 32 + tid];
    }
  }
  for (; qt < n_q; qt = qt_next) {
    const int q0 = qt * 32;
    __syncthreads();
    st.store(q_lds, qv8);
    st.store(do_lds, dv8);
    if (side_ld) {
      lse_lds[tid] = lse_n;
      dd_lds[tid] = dd_n;
      if constexpr (SEG) seg_lds[tid] = sq_n;
    }
    __syncthreads();
    qt_next = live.next(qt + 1, n_q);
    if (qt_next < n_q) {
      qv8 = st.load(q + qkv_off, qt_next * 32, g.qkv_rs);
      dv8 = st.load(dout + o_off, qt_next * 32, g.o_rs);
      if (side_ld) {
        lse_n = lse[(long)bh * L + qt_next * 32 + tid];
        dd_n = ddot[(long)bh * L + qt_next * 32 + tid];
        if constexpr (SEG) sq_n = srow[qt_next * 32 + tid];
      }
    }

    if (wave_skip) continue;
    // q segment ids of the staged tile, by register row; a tile that holds
    // none of this wave's kv segments contributes exact zeros
    int sq_r[16];
    if constexpr (SEG) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sq_r[r] = seg_lds[c_row(r, half)];
      if (!fa_seg_tile_live(sq_r, sk, sk)) continue;
    }
    // S[q, kv] and dP[q, kv]: reg=q rows, lane=kv cols
    f32x16 s_acc = (f32x16)(0.f);
    f32x16 dp_acc = (f32x16)(0.f);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      short8_t qfrag = tile_row_frag(q_lds, col, half, c);
      short8_t dofrag = tile_row_frag(do_lds, col, half, c);
      s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfrag, kf[c], s_acc,
                                                      0, 0, 0);
      dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dofrag, vf[c], dp_acc,
                                                       0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);

    // elementwise (lse/ddot by register row, mask bias one scalar per lane)
    float pv[16], gv[16];
    unsigned keep = 0;
    if constexpr (DROP)
      keep = fa_drop_keep16_qreg(dr, dblk, drop_nb, q0 / 4 + half, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int ql = c_row(r, half);
      float bias = mb;
      if constexpr (SEG) bias = sq_r[r] == sk ? 0.f : FA_SEG_BIAS;
      const float p = __expf(s_acc[r] * scale + bias - lse_lds[ql]);
      if constexpr (DROP) {
        const bool kept = (keep >> r) & 1u;
        pv[r] = kept ? p : 0.f;
        gv[r] = scale * p * ((kept ? dp_acc[r] * dr.scale : 0.f) - dd_lds[ql]);
      } else {
        pv[r] = p;
        gv[r] = scale * pv[r] * (dp_acc[r] - dd_lds[ql]);
      }
    }
    // dS out, natural [q, kv] rows (2 B per lane, lanes contiguous in kv);
    // only on the A/B path that feeds flash_dq_kernel
    if (!SEG && ds != nullptr && kv_valid) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ds[bh_sq + (long)(q0 + c_row(r, half)) * L + my_kv] =
            f32_to_bf16(gv[r]);
    }

    // repack P and dS to A-fragments [row=kv][k=q]
    short8_t pf[2], gf[2];
    c_to_afrag2(pv, pf, gv, gf);

    // dO^T and Q^T B-fragments [row=d][k=q], then the two accumulation
    // chains (reg=kv rows, lane=d cols)
    FaTrFrags doT, qT;
    tr_issue(do_lds, tro, doT);
    tr_gather(q_lds, tro, qT);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        dv_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            pf[c], doT.frag(c, t), dv_acc[t], 0, 0, 0);
        dk_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            gf[c], qT.frag(c, t), dk_acc[t], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }
  }   // !skip_tile

  // epilogue: dV/dK rows of this wave's kv block (reg=kv row, lane=d col)
  float csk[2] = {0.f, 0.f}, csv[2] = {0.f, 0.f};   // BIAS: column sums
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int kvl = c_row(r, half);
      if (kv_base + kvl >= L) continue;
      long off = qkv_off + (long)(kv_base + kvl) * g.qkv_rs + 32 * t + col;
      const short vb =
          f32_to_bf16(DROP ? dv_acc[t][r] * dr.scale : dv_acc[t][r]);
      const short kb16 = f32_to_bf16(dk_acc[t][r]);
      dv[off] = vb;
      dk[off] = kb16;
      if constexpr (BIAS) {   // the sum of what is STORED
        csv[t] += bf16_to_f32(vb);
        csk[t] += bf16_to_f32(kb16);
      }
    }
  }
  // folded bias gradient: this workgroup's k and v columns of its ws row.
  // The barriers are unconditional, so workgroup-uniform; skip_tile and
  // wave_skip arrive here with exact-zero accumulators, rows past L add
  // nothing.
  if constexpr (BIAS) {
    float* cs = (float*)smem;        // [2][FA_WAVES][64]: dK, dV
    __syncthreads();                 // every wave is done with the tiles
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float sk_ = fa_half_merge(csk[t]);
      float sv_ = fa_half_merge(csv[t]);
      if (half == 0) {
        cs[(0 * FA_WAVES + wid) * FA_DH + 32 * t + col] = sk_;
        cs[(1 * FA_WAVES + wid) * FA_DH + 32 * t + col] = sv_;
      }
    }
    __syncthreads();
    const int third = bias_ld / 3;
    float* row = bias_ws + ((long)b * n_kvblocks + kb) * bias_ld + h * FA_DH;
    fa_colsum_merge_store(cs, tid, row + third, row + 2 * third);
  }
}

static void fa_bwd_fused_dispatch(const short* q, const short* k,
                                  const short* v, const void* dout,
                                  const void* mask, const void* seg,
                                  const void* lse, const void* ddot,
                                  const void* dead, void* ds,
                                  short* dk, short* dv, int B, int H, int L,
                                  float scale, FaGeom g, float* bias_ws,
                                  FaDrop dr, hipStream_t stream) {
  const dim3 grid = fa_grid(B, H, L, FA_QWG);
  const int bias_ld = 3 * H * FA_DH;
#define FA_BWD_SEG_ARGS                                                       \
  q, k, v, (const short*)dout, nullptr, (const int*)seg, (const float*)lse,   \
      (const float*)ddot, (const unsigned char*)dead, nullptr, dk, dv, B, H,  \
      L, scale, g, bias_ws, bias_ld, dr
#define FA_BWD_ARGS                                                           \
  q, k, v, (const short*)dout, (const float*)mask, nullptr,                   \
      (const float*)lse, (const float*)ddot, (const unsigned char*)dead,      \
      (short*)ds, dk, dv, B, H, L, scale, g, bias_ws, bias_ld, dr
  // the callers have refused dropout with bias_ws or ds
  if (seg && dr.thr) {
    flash_bwd_fused_kernel<true, false, true>
        <<<grid, FA_BLOCK, BWD_SEG_LDS_BYTES, stream>>>(FA_BWD_SEG_ARGS);
  } else if (dr.thr) {
    flash_bwd_fused_kernel<false, false, true>
        <<<grid, FA_BLOCK, BWD_LDS_BYTES, stream>>>(FA_BWD_ARGS);
  } else if (seg && bias_ws) {
    flash_bwd_fused_kernel<true, true, false>
        <<<grid, FA_BLOCK, BWD_SEG_LDS_BYTES, stream>>>(FA_BWD_SEG_ARGS);
  } else if (seg) {
    flash_bwd_fused_kernel<true, false, false>
        <<<grid, FA_BLOCK, BWD_SEG_LDS_BYTES, stream>>>(FA_BWD_SEG_ARGS);
  } else if (bias_ws) {
    flash_bwd_fused_kernel<false, true, false>
        <<<grid, FA_BLOCK, BWD_LDS_BYTES, stream>>>(FA_BWD_ARGS);
  } else {
    flash_bwd_fused_kernel<false, false, false>
        <<<grid, FA_BLOCK, BWD_LDS_BYTES, stream>>>(FA_BWD_ARGS);
  }
#undef FA_BWD_ARGS
#undef FA_BWD_SEG_ARGS
}

// seg and dropout exclude the dS output: with either given, ds must be
// nullptr.  dead is ignored when ds is given.
extern "C" hipError_t flash_bwd_fused_launch(
    const void* q, const void* k, const void* v, const void* dout,
    const void* mask, const void* seg, const void* lse, const void* ddot,
    const void* dead, void* ds, void* dk, void* dv, int B, int H, int L,
    float scale, unsigned long long drop_seed, unsigned drop_call,
    unsigned drop_site, unsigned drop_thr, hipStream_t stream) {
  if ((seg || drop_thr) && ds) return hipErrorInvalidValue;
  if (!fa_drop_ok(drop_thr)) return hipErrorInvalidValue;
  fa_bwd_fused_dispatch((const short*)q, (const short*)k, (const short*)v,
                        dout, mask, seg, lse, ddot, dead, ds, (short*)dk,
                        (short*)dv, B, H, L, scale, FaGeom::bhld(H, L),
                        nullptr,
                        fa_drop_make(drop_seed, drop_call, drop_site, drop_thr),
                        stream);
  return hipGetLastError();
}

// packed: qkv/dqkv [B, L, 3D], dout [B, L, D]; dk/dv land inside dqkv.
// bias_ws (optional): [flash_bias_ws_rows(B, L), 3D] f32 column partials, the
// k and v thirds are written here.
extern "C" hipError_t flash_bwd_fused_packed_launch(
    const void* qkv, const void* dout, const void* mask, const void* seg,
    const void* lse, const void* ddot, const void* dead, void* dqkv,
    void* bias_ws, int B, int H, int L, float scale,
    unsigned long long drop_seed, unsigned drop_call, unsigned drop_site,
    unsigned drop_thr, hipStream_t stream) {
  if (drop_thr && bias_ws) return hipErrorInvalidValue;
  if (!fa_drop_ok(drop_thr)) return hipErrorInvalidValue;
  const int D = H * FA_DH;
  fa_bwd_fused_dispatch((const short*)qkv, (const short*)qkv + D,
                        (const short*)qkv + 2 * D, dout, mask, seg, lse, ddot,
                        dead, nullptr, (short*)dqkv + D, (short*)dqkv + 2 * D, B, H,
                        L, scale, FaGeom::packed(H, L), (float*)bias_ws,
                        fa_drop_make(drop_seed, drop_call, drop_site, drop_thr),
                        stream);
  return hipGetLastError();
}

// dQ = dS @ K from a materialized dS — a purpose-built kernel instead of a
// library bmm ([L, L] x [L, 64] batched shapes run at ~225 TF in
// hipBLASLt).  Structure mirrors flash_fwd's PV stage: two independent
// 32-row q-blocks per wave (ILP), dS rows read straight from HBM as MFMA
// A-fragments (contiguous short8 per lane), K tiles staged swizzled in LDS
// and gathered as K^T B-fragments.  ds/k/dq are [B, H, L, *] contiguous.
extern "C" __global__ void __launch_bounds__(FA_BLOCK, 2)
flash_dq_kernel(const short* __restrict__ ds, const short* __restrict__ k,
                short* __restrict__ dq, int B, int H, int L) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* k_lds = (short*)smem;

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int col = lane & 31;
  const int half = lane >> 5;
  const FaTrOffsets tro = tr_offsets(lane, half);

  const FaQBlocks qb = fa_qblocks(L, wid);
  const long bh_off = (long)qb.bh * L * FA_DH;
  const long bh_sq = (long)qb.bh * L * L;
  const int my_qA = min(qb.qA + col, L - 1);
  const int my_qB = min(qb.qB + col, L - 1);
  const short* dsA_row = ds + bh_sq + (long)my_qA * L;
  const short* dsB_row = ds + bh_sq + (long)my_qB * L;

  f32x16 oA[2], oB[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { oA[t] = (f32x16)(0.f); oB[t] = (f32x16)(0.f); }

  const int n_kv = L / FA_KVB;
  const FaStager st(tid);
  short8_t kv8 = st.load(k + bh_off, 0, FA_DH);
  for (int kt = 0; kt < n_kv; ++kt) {
    const int kv0 = kt * FA_KVB;
    __syncthreads();
    st.store(k_lds, kv8);
    __syncthreads();
    if (kt + 1 < n_kv) kv8 = st.load(k + bh_off, kv0 + FA_KVB, FA_DH);
    // dS A-fragments straight from HBM: lane reads its q row's kv chunk
    short8_t aA[2], aB[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      aA[c] = *(const short8_t*)(dsA_row + kv0 + 16 * c + 8 * half);
      aB[c] = *(const short8_t*)(dsB_row + kv0 + 16 * c + 8 * half);
    }
    FaTrFrags kT;
    tr_gather(k_lds, tro, kT);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        short8_t kf = kT.frag(c, t);
        oA[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aA[c], kf, oA[t],
                                                        0, 0, 0);
        oB[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aB[c], kf, oB[t],
                                                        0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int rloc = c_row(r, half);
      int qA = qb.qA + rloc, qB = qb.qB + rloc;
      if (qA < L)
        dq[bh_off + (long)qA * FA_DH + 32 * t + col] = f32_to_bf16(oA[t][r]);
      if (qB < L)
        dq[bh_off + (long)qB * FA_DH + 32 * t + col] = f32_to_bf16(oB[t][r]);
    }
  }
}

extern "C" hipError_t flash_dq_launch(const void* ds, const void* k, void* dq,
                                      int B, int H, int L,
                                      hipStream_t stream) {
  flash_dq_kernel<<<fa_grid(B, H, L, FA_Q2WG), FA_BLOCK, DQ_LDS_BYTES,
                    stream>>>(
      (const short*)ds, (const short*)k, (short*)dq, B, H, L);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// dQ by recompute: forward-orientation kernel that recomputes S = QK^T and
// dP = dO V^T per kv tile, forms dS in registers and accumulates
// dQ = dS @ K — no dS materialization at all.  Against the
// flash_bwd_fused(emit dS) + flash_dq pair this saves the [B, H, L, L]
// bf16 dS HBM round-trip (1.07 GB written + 1.07 GB re-read at the bench
// shape).
//
// Structure mirrors flash_fwd exactly (two independent 32-row q-blocks per
// wave for ILP; K/V tiles staged swizzled in LDS, double-staged across the
// kv loop):
//   S  C-layout (reg=kv, lane=q) from mfma(A=K-frag, B=Q-rows)
//   dP C-layout (reg=kv, lane=q) from mfma(A=V-frag, B=dO-rows)
//   lse/ddot are LANE-local scalars (one q row per lane), the mask bias
//   indexes by the kv REGISTER — both orientations line up for free
//   dS = scale * P * (dP - D) in registers
//   dS -> A-fragments [row=q][k=kv]
//   dQ[q, d] += mfma(dS-frag, K^T-frag), K^T gathered from the staged K tile
// Segmented (SEG): as in flash_fwd — q ids lane-local, kv ids per register,
// kv tiles limited to the workgroup's fa_seg_range.
// Dropout (DROP, never with BIAS): dS = scale * P * (keep * drop_scale * dP
// - D), the mask drawn as in flash_fwd (same layout, same call).
template <bool SEG, bool BIAS, bool DROP>
__global__ void __launch_bounds__(FA_BLOCK, FA_DQR_WAVES(DROP))
flash_dq_recompute_kernel(const short* __restrict__ q,
                          const short* __restrict__ k,
                          const short* __restrict__ v,
                          const short* __restrict__ dout,
                          const float* __restrict__ mask,
                          const int* __restrict__ seg,
                          const float* __restrict__ lse,
                          const float* __restrict__ ddot,
                          const unsigned char* __restrict__ dead,
                          short* __restrict__ dq,
                          int B, int H, int L, float scale, FaGeom g,
                          float* __restrict__ bias_ws, int bias_ld,
                          FaDrop dr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* k_lds = (short*)smem;
  short* v_lds = (short*)(smem + TILE_LDS_BYTES);
  float* mb_lds = (float*)(smem + 2 * TILE_LDS_BYTES);   // side [32]
  int* sk_lds = (int*)mb_lds;
  int* skip_scratch = (int*)(smem + 2 * TILE_LDS_BYTES + SIDE_LDS_BYTES);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int col = lane & 31;
  const int half = lane >> 5;
  const FaTrOffsets tro = tr_offsets(lane, half);

  const FaQBlocks qb = fa_qblocks(L, wid);
  const int b = qb.bh / H;
  const int h = qb.bh % H;
  const long qkv_off = (long)b * g.qkv_bs + (long)h * g.qkv_hs;
  const long o_off = (long)b * g.o_bs + (long)h * g.o_hs;

  // Dead query tiles (all-zero dO, see above): lanes 0..7 fetch the
  // flags of the workgroup's eight tiles; a tile past L counts as dead.  The
  // byte is loaded first and looked at only after the q/dO loads below are
  // issued, so its latency is not ahead of theirs.
  bool tile_dead = false;
  if (dead) {
    const int n_t = L / FA_QB;
    const int t = (qb.qA - wid * FA_QB) / FA_QB + lane;
    tile_dead = lane < 8 && (t >= n_t || dead[(long)qb.bh * n_t + t] != 0);
  }

  const int my_qA = qb.qA + col;
  const int my_qB = qb.qB + col;
  const bool validA = my_qA < L;
  const bool validB = my_qB < L;
  const float* mrow = (!SEG && mask) ? mask + (long)b * L : nullptr;
  const int* srow = SEG ? seg + (long)b * L : nullptr;
  int sqA = 0, sqB = 0;
  if constexpr (SEG) {
    sqA = srow[validA ? my_qA : L - 1];
    sqB = srow[validB ? my_qB : L - 1];
  }

  short8_t qfA[4], qfB[4], dofA[4], dofB[4];
  {
    const short* qrA = q + qkv_off + (long)(validA ? my_qA : L - 1) * g.qkv_rs;
    const short* qrB = q + qkv_off + (long)(validB ? my_qB : L - 1) * g.qkv_rs;
    const short* drA = dout + o_off + (long)(validA ? my_qA : L - 1) * g.o_rs;
    const short* drB = dout + o_off + (long)(validB ? my_qB : L - 1) * g.o_rs;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      qfA[c] = *(const short8_t*)(qrA + c * 16 + half * 8);
      qfB[c] = *(const short8_t*)(qrB + c * 16 + half * 8);
      dofA[c] = *(const short8_t*)(drA + c * 16 + half * 8);
      dofB[c] = *(const short8_t*)(drB + c * 16 + half * 8);
    }
  }
  const float lseA = lse[(long)qb.bh * L + (validA ? my_qA : L - 1)];
  const float lseB = lse[(long)qb.bh * L + (validB ? my_qB : L - 1)];
  const float ddA = ddot[(long)qb.bh * L + (validA ? my_qA : L - 1)];
  const float ddB = ddot[(long)qb.bh * L + (validB ? my_qB : L - 1)];
  // DROP: the mask blocks of this lane's two q rows, block column 0
  unsigned long long dblkA = 0, dblkB = 0;
  if constexpr (DROP) {
    const unsigned long long nb = (unsigned)L / 4;
    dblkA = ((unsigned long long)qb.bh * nb + (unsigned)(my_qA >> 2)) * nb;
    dblkB = ((unsigned long long)qb.bh * nb + (unsigned)(my_qB >> 2)) * nb;
  }

  // bit i of dmask = tile i dead; wave wid owns bits wid (block A) and
  // 4 + wid (block B).  A dead tile's dQ rows are exact zeros.
  const unsigned dmask = (unsigned)__builtin_amdgcn_ballot_w64(tile_dead);
  // All eight dead: zero rows (and zero q-third bias partials), no K/V load.
  // dmask is workgroup-uniform, so leaving before the barriers is safe.
  if (dmask == 0xffu) {
    fa_store_zero_tile(dq + qkv_off, g.qkv_rs, qb.qA, L, lane);
    fa_store_zero_tile(dq + qkv_off, g.qkv_rs, qb.qB, L, lane);
    if constexpr (BIAS) {
      if (tid < 2 * FA_DH) {
        const int n128 = (L + FA_QWG - 1) / FA_QWG;
        const int blk = (qb.qA - wid * FA_QB) / FA_QWG + tid / FA_DH;
        if (blk < n128)
          bias_ws[((long)b * n128 + blk) * bias_ld + h * FA_DH + tid % FA_DH] =
              0.f;
      }
    }
    return;
  }
  // Both blocks of this wave dead: it keeps staging and keeps the barriers,
  // skips the MFMA and softmax work, and its zero accumulators are stored by
  // the common epilogue.
  const bool wave_dead = ((dmask >> wid) & 0x11u) == 0x11u;

  f32x16 dqA[2], dqB[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { dqA[t] = (f32x16)(0.f); dqB[t] = (f32x16)(0.f); }

  const int n_kv = L / FA_KVB;
  int kt_begin = 0;
  int n_kv_eff = n_kv;
  if (mrow) {
    int last = fa_last_active_kv(mrow, L, tid, skip_scratch);
    if (last >= 0) n_kv_eff = min(n_kv, last / FA_KVB + 1);
  }
  if constexpr (SEG) {
    const int q_lo = qb.qA - wid * FA_QB;        // the workgroup's first q row
    const FaRange kr = fa_seg_range(srow, L, q_lo, min(q_lo + FA_Q2WG, L) - 1,
                                    tid, skip_scratch);
    kt_begin = kr.lo / FA_KVB;
    n_kv_eff = kr.hi / FA_KVB + 1;
  }
  const FaStager st(tid);
  short8_t kv8 = st.load(k + qkv_off, kt_begin * FA_KVB, g.qkv_rs);
  short8_t vv8 = st.load(v + qkv_off, kt_begin * FA_KVB, g.qkv_rs);
  // the tile's side word (fa_side_rows), threads 0..31
  const bool side_ld = (SEG || mrow) && tid < FA_KVB;
  float mb_n = 0.f;
  int sk_n = 0;
  if (side_ld) {
    if constexpr (SEG) sk_n = srow[kt_begin * FA_KVB + tid];
    else mb_n = mrow[kt_begin * FA_KVB + tid];
  }
  for (int kt = kt_begin; kt < n_kv_eff; ++kt) {
    const int kv0 = kt * FA_KVB;
    __syncthreads();
    st.store(k_lds, kv8);
    st.store(v_lds, vv8);
    if (side_ld) {
      if constexpr (SEG) sk_lds[tid] = sk_n;
      else mb_lds[tid] = mb_n;
    }
    __syncthreads();
    if (kt + 1 < n_kv_eff) {
      kv8 = st.load(k + qkv_off, kv0 + FA_KVB, g.qkv_rs);
      vv8 = st.load(v + qkv_off, kv0 + FA_KVB, g.qkv_rs);
      if (side_ld) {
        if constexpr (SEG) sk_n = srow[kv0 + FA_KVB + tid];
        else mb_n = mrow[kv0 + FA_KVB + tid];
      }
    }
    if (wave_dead) continue;

    float mb_r[16];
    int sk_r[16];
    if constexpr (SEG) {
      fa_side_rows(sk_lds, half, sk_r);
    } else if (mrow) {
      fa_side_rows(mb_lds, half, mb_r);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) mb_r[r] = 0.f;
    }
    if constexpr (SEG) {
      if (!fa_seg_tile_live(sk_r, sqA, sqB)) continue;
    }

    // ---- S and dP for BOTH q-blocks (16 back-to-back MFMAs) ----
    f32x16 sA = (f32x16)(0.f), sB = (f32x16)(0.f);
    f32x16 pA = (f32x16)(0.f), pB = (f32x16)(0.f);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      short8_t kf = tile_row_frag(k_lds, col, half, c);
      short8_t vf = tile_row_frag(v_lds, col, half, c);
      sA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfA[c], sA, 0, 0, 0);
      sB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qfB[c], sB, 0, 0, 0);
      pA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dofA[c], pA, 0, 0, 0);
      pB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dofB[c], pB, 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- dS in registers (lse/ddot lane-local, mask by kv register) ----
    float gA[16], gB[16];
    unsigned keepA = 0, keepB = 0;
    if constexpr (DROP) {
      keepA = fa_drop_keep16_kvreg(dr, dblkA, kv0 / 4 + half, lane);
      keepB = fa_drop_keep16_kvreg(dr, dblkB, kv0 / 4 + half, lane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float mbA, mbB;
      if constexpr (SEG) {
        mbA = sk_r[r] == sqA ? 0.f : FA_SEG_BIAS;
        mbB = sk_r[r] == sqB ? 0.f : FA_SEG_BIAS;
      } else {
        mbA = mbB = mb_r[r];
      }
      float expA = __expf(sA[r] * scale + mbA - lseA);
      float expB = __expf(sB[r] * scale + mbB - lseB);
      float dpA = pA[r], dpB = pB[r];
      if constexpr (DROP) {
        dpA = (keepA >> r) & 1u ? dpA * dr.scale : 0.f;
        dpB = (keepB >> r) & 1u ? dpB * dr.scale : 0.f;
      }
      gA[r] = scale * expA * (dpA - ddA);
      gB[r] = scale * expB * (dpB - ddB);
    }

    // ---- dS -> A-fragments [row=q][k=kv] ----
    short8_t gfA[2], gfB[2];
    c_to_afrag2(gA, gfA, gB, gfB);

    // ---- dQ += dS @ K via tr_b16-gathered K^T fragments ----
    FaTrFrags kT;
    tr_gather(k_lds, tro, kT);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        short8_t kf = kT.frag(c, t);
        dqA[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gfA[c], kf, dqA[t],
                                                         0, 0, 0);
        dqB[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gfB[c], kf, dqB[t],
                                                         0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue ----
  float csA[2] = {0.f, 0.f}, csB[2] = {0.f, 0.f};   // BIAS: column sums
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int rloc = c_row(r, half);
      int qA = qb.qA + rloc, qB = qb.qB + rloc;
      if (qA < L) {
        const short a16 = f32_to_bf16(dqA[t][r]);
        dq[qkv_off + (long)qA * g.qkv_rs + 32 * t + col] = a16;
        if constexpr (BIAS) csA[t] += bf16_to_f32(a16);   // what is STORED
      }
      if (qB < L) {
        const short b16 = f32_to_bf16(dqB[t][r]);
        dq[qkv_off + (long)qB * g.qkv_rs + 32 * t + col] = b16;
        if constexpr (BIAS) csB[t] += bf16_to_f32(b16);
      }
    }
  }
  // folded bias gradient: the q columns of the two 128-row blocks this
  // workgroup covers (the waves' A blocks, then their B blocks).  The
  // barriers are unconditional, so workgroup-uniform.
  if constexpr (BIAS) {
    float* cs = (float*)smem;        // [2][FA_WAVES][64]: blocks A, B
    __syncthreads();                 // every wave is done with the tiles
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float sA_ = fa_half_merge(csA[t]);
      float sB_ = fa_half_merge(csB[t]);
      if (half == 0) {
        cs[(0 * FA_WAVES + wid) * FA_DH + 32 * t + col] = sA_;
        cs[(1 * FA_WAVES + wid) * FA_DH + 32 * t + col] = sB_;
      }
    }
    __syncthreads();
    const int n128 = (L + FA_QWG - 1) / FA_QWG;
    const int blkA = (qb.qA - wid * FA_QB) / FA_QWG;   // workgroup-uniform
    float* row = bias_ws + ((long)b * n128 + blkA) * bias_ld + h * FA_DH;
    fa_colsum_merge_store(cs, tid, row,
                          blkA + 1 < n128 ? row + bias_ld : nullptr);
  }
}

static void fa_dq_recompute_dispatch(const short* q, const short* k,
                                     const short* v, const void* dout,
                                     const void* mask, const void* seg,
                                     const void* lse, const void* ddot,
                                     const void* dead, void* dq, int B, int H,
                                     int L, float scale, FaGeom g,
                                     float* bias_ws, FaDrop dr,
                                     hipStream_t stream) {
  const dim3 grid = fa_grid(B, H, L, FA_Q2WG);
  const int bias_ld = 3 * H * FA_DH;
#define FA_DQR_SEG_ARGS                                                       \
  q, k, v, (const short*)dout, nullptr, (const int*)seg, (const float*)lse,   \
      (const float*)ddot, (const unsigned char*)dead, (short*)dq, B, H, L,    \
      scale, g, bias_ws, bias_ld, dr
#define FA_DQR_ARGS                                                           \
  q, k, v, (const short*)dout, (const float*)mask, nullptr,                   \
      (const float*)lse, (const float*)ddot, (const unsigned char*)dead,      \
      (short*)dq, B, H, L, scale, g, bias_ws, bias_ld, dr
  // the callers have refused dropout with bias_ws
  if (seg && dr.thr) {
    flash_dq_recompute_kernel<true, false, true>
        <<<grid, FA_BLOCK, DQR_LDS_BYTES, stream>>>(FA_DQR_SEG_ARGS);
  } else if (dr.thr) {
    flash_dq_recompute_kernel<false, false, true>
        <<<grid, FA_BLOCK, DQR_LDS_BYTES, stream>>>(FA_DQR_ARGS);
  } else if (seg && bias_ws) {
    flash_dq_recompute_kernel<true, true, false>
        <<<grid, FA_BLOCK, DQR_LDS_BYTES, stream>>>(FA_DQR_SEG_ARGS);
  } else if (seg) {
    flash_dq_recompute_kernel<true, false, false>
        <<<grid, FA_BLOCK, DQR_LDS_BYTES, stream>>>(FA_DQR_SEG_ARGS);
  } else if (bias_ws) {
    flash_dq_recompute_kernel<false, true, false>
        <<<grid, FA_BLOCK, DQR_LDS_BYTES, stream>>>(FA_DQR_ARGS);
  } else {
    flash_dq_recompute_kernel<false, false, false>
        <<<grid, FA_BLOCK, DQR_LDS_BYTES, stream>>>(FA_DQR_ARGS);
  }
#undef FA_DQR_ARGS
#undef FA_DQR_SEG_ARGS
}

extern "C" hipError_t flash_dq_recompute_launch(
    const void* q, const void* k, const void* v, const void* dout,
    const void* mask, const void* seg, const void* lse, const void* ddot,
    const void* dead, void* dq, int B, int H, int L, float scale,
    unsigned long long drop_seed, unsigned drop_call, unsigned drop_site,
    unsigned drop_thr, hipStream_t stream) {
  if (!fa_drop_ok(drop_thr)) return hipErrorInvalidValue;
  fa_dq_recompute_dispatch((const short*)q, (const short*)k, (const short*)v,
                           dout, mask, seg, lse, ddot, dead, dq, B, H, L, scale,
                           FaGeom::bhld(H, L), nullptr,
                           fa_drop_make(drop_seed, drop_call, drop_site,
                                        drop_thr),
                           stream);
  return hipGetLastError();
}

// packed: dq lands in the q third of dqkv [B, L, 3D]; bias_ws (optional) as
// in flash_bwd_fused_packed_launch, the q third is written here.
extern "C" hipError_t flash_dq_recompute_packed_launch(
    const void* qkv, const void* dout, const void* mask, const void* seg,
    const void* lse, const void* ddot, const void* dead, void* dqkv,
    void* bias_ws, int B, int H, int L, float scale,
    unsigned long long drop_seed, unsigned drop_call, unsigned drop_site,
    unsigned drop_thr, hipStream_t stream) {
  if (drop_thr && bias_ws) return hipErrorInvalidValue;
  if (!fa_drop_ok(drop_thr)) return hipErrorInvalidValue;
  const int D = H * FA_DH;
  fa_dq_recompute_dispatch((const short*)qkv, (const short*)qkv + D,
                           (const short*)qkv + 2 * D, dout, mask, seg, lse,
                           ddot, dead, dqkv, B, H, L, scale,
                           FaGeom::packed(H, L), (float*)bias_ws,
                           fa_drop_make(drop_seed, drop_call, drop_site,
                                        drop_thr),
                           stream);
  return hipGetLastError();
}

// D = rowsum(dO * O) and the dead-tile flags, from one read of dO.
//
// One wave owns one 32-row query tile of one (b, h): eight passes of four
// rows, 16 lanes x 4 bf16 per 64-element row, each row's dot product reduced
// across its 16-lane group in a fixed order.  All sixteen loads of a lane
// are issued before the first is used.
//
// dead[tile] = 1 iff every one of the tile's 32 x 64 dO elements is +-0
// ((bits & 0x7fff) == 0), else 0: a plain store by lane 0 on every call, so
// no memset and no state between calls.  For such a tile dP, D and dS are
// exact zeros whatever P is (finite inputs), which is what lets the two
// backward kernels skip it — see docs/KERNELS.md.
__device__ __forceinline__ float fa_row_dot(short4_t a, short4_t c) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += bf16_to_f32(a[j]) * bf16_to_f32(c[j]);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
  return s;
}

// dr/orow: row 0 of the tile, rows `rs` shorts apart; dd: the tile's 32 ddot
// slots; n_valid: rows of the tile that exist (32 unless the tile is the
// partial last one of a flat [n_rows, 64] tensor).
__device__ __forceinline__ void fa_dot_tile(const short* dr, const short* orow,
                                            long rs, float* dd,
                                            unsigned char* dead_flag,
                                            int n_valid, int lane) {
  const int sub = lane & 15, grp = lane >> 4;
  short4_t a[8], c[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int r = min(4 * p + grp, n_valid - 1);
    a[p] = *(const short4_t*)(dr + r * rs + sub * 4);
    c[p] = *(const short4_t*)(orow + r * rs + sub * 4);
  }
  unsigned nz = 0;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int r = 4 * p + grp;
    const float s = fa_row_dot(a[p], c[p]);
    if (r < n_valid) {
#pragma unroll
      for (int j = 0; j < 4; ++j) nz |= (unsigned)a[p][j] & 0x7fffu;
      if (sub == 0) dd[r] = s;
    }
  }
  const bool live = __builtin_amdgcn_ballot_w64(nz != 0) != 0;
  if (lane == 0) *dead_flag = live ? 0 : 1;
}

// dout/o [n_rows, 64] (any [B, H, L, 64]); ddot [n_rows]; dead
// [ceil(n_rows / 32)], = [B, H, L / 32] when L % 32 == 0.
extern "C" __global__ void __launch_bounds__(FA_BLOCK)
fa_dot_kernel(const short* __restrict__ dout, const short* __restrict__ o,
              float* __restrict__ ddot, unsigned char* __restrict__ dead,
              long n_rows) {
  const long tile = (long)blockIdx.x * FA_WAVES + threadIdx.x / WAVE;
  const long row0 = tile * FA_QB;
  if (row0 >= n_rows) return;                       // wave-uniform
  fa_dot_tile(dout + row0 * FA_DH, o + row0 * FA_DH, FA_DH, ddot + row0,
              dead + tile, (int)min((long)FA_QB, n_rows - row0),
              threadIdx.x & (WAVE - 1));
}

// packed fa_dot: dout/o are [B, L, D] (D = H*64); ddot is [B, H, L], dead
// [B, H, L / 32].  Wave -> (b, tile, h), h fastest, so the waves of a
// workgroup read neighbouring 128-B pieces of the same rows.
extern "C" __global__ void __launch_bounds__(FA_BLOCK)
fa_dot_packed_kernel(const short* __restrict__ dout,
                     const short* __restrict__ o, float* __restrict__ ddot,
                     unsigned char* __restrict__ dead, int B, int H, int L) {
  const int D = H * FA_DH;
  const int n_t = L / FA_QB;
  const long wv = (long)blockIdx.x * FA_WAVES + threadIdx.x / WAVE;
  if (wv >= (long)B * n_t * H) return;              // wave-uniform
  const int h = (int)(wv % H);
  const long bt = wv / H;                           // b * n_t + tile
  const int t = (int)(bt % n_t);
  const long b = bt / n_t;
  const long in_off = (b * L + (long)t * FA_QB) * D + h * FA_DH;
  const long bh = b * H + h;
  fa_dot_tile(dout + in_off, o + in_off, D, ddot + bh * L + t * FA_QB,
              dead + bh * n_t + t, FA_QB, threadIdx.x & (WAVE - 1));
}

extern "C" hipError_t fa_dot_packed_launch(const void* dout, const void* o,
                                           void* ddot, void* dead, int B,
                                           int H, int L, hipStream_t stream) {
  const long waves = (long)B * H * (L / FA_QB);
  const int grid = (int)((waves + FA_WAVES - 1) / FA_WAVES);
  fa_dot_packed_kernel<<<grid, FA_BLOCK, 0, stream>>>(
      (const short*)dout, (const short*)o, (float*)ddot, (unsigned char*)dead,
      B, H, L);
  return hipGetLastError();
}

extern "C" hipError_t fa_dot_launch(const void* dout, const void* o,
                                    void* ddot, void* dead, long n_rows,
                                    hipStream_t stream) {
  const long waves = (n_rows + FA_QB - 1) / FA_QB;
  const int grid = (int)((waves + FA_WAVES - 1) / FA_WAVES);
  fa_dot_kernel<<<grid, FA_BLOCK, 0, stream>>>(
      (const short*)dout, (const short*)o, (float*)ddot, (unsigned char*)dead,
      n_rows);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// ds_read_b64_tr_b16 semantics probe (development aid, exposed for tests):
// stage `src` (bf16, 256 elements) into LDS, then each lane issues the
// transpose-read at a caller-chosen address scheme and writes its 4 bf16
// results to out[lane][0..3].
//   scheme 0: addr = 0 for every lane
//   scheme 1: addr = (lane & 15) * 2
//   scheme 2: addr = ((lane & 15) + (lane >> 4) * 64) * 2
//   scheme 3: addr = (lane >> 4) * 128  (16-lane-group base, uniform in group)
extern "C" __global__ void __launch_bounds__(64)
tr_probe_kernel(const short* __restrict__ src, short* __restrict__ out,
                int scheme) {
  __shared__ __attribute__((aligned(16))) short lds[256];
  int lane = threadIdx.x;
  for (int i = lane; i < 256; i += 64) lds[i] = src[i];
  __syncthreads();
  int addr;
  switch (scheme) {
    case 0: addr = 0; break;
    case 1: addr = (lane & 15) * 2; break;
    case 2: addr = ((lane & 15) + (lane >> 4) * 64) * 2; break;
    case 3: addr = (lane >> 4) * 128; break;
    case 4: addr = (lane & 3) * 16; break;           // mates' ~3-bases differ
    case 5: addr = ((lane & 3) * 32 + 4 * ((lane >> 2) & 7)) * 2; break;
    case 6: addr = ((lane & 3) * 8 + 4) * 2; break;
    // one-mate-at-a-time base perturbation (which mate feeds which output?)
    case 7: addr = ((lane & 3) == 0) ? 16 : 0; break;
    case 8: addr = ((lane & 3) == 1) ? 16 : 0; break;
    case 9: addr = ((lane & 3) == 2) ? 16 : 0; break;
    case 10: addr = ((lane & 3) == 3) ? 16 : 0; break;
    // kernel-like: row stride 64 elems per mate + d-quad by quad index
    case 11: addr = ((lane & 3) * 64 + 4 * ((lane >> 2) & 7)) * 2; break;
    // distinct per mate AND per quad
    default: addr = ((lane & 3) * 8 + ((lane >> 2) & 7) * 32) * 2; break;
  }
  typedef __attribute__((ext_vector_type(2))) unsigned uint2_t;
  uint2_t r;
  unsigned base = (unsigned)(unsigned long)((char*)lds + addr);
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)"
               : "=v"(r) : "v"(base) : "memory");
  __builtin_amdgcn_sched_barrier(0);
  out[lane * 4 + 0] = (short)(r[0] & 0xffff);
  out[lane * 4 + 1] = (short)(r[0] >> 16);
  out[lane * 4 + 2] = (short)(r[1] & 0xffff);
  out[lane * 4 + 3] = (short)(r[1] >> 16);
}

extern "C" hipError_t tr_probe_launch(const void* src, void* out, int scheme,
                                      hipStream_t stream) {
  tr_probe_kernel<<<1, 64, 0, stream>>>((const short*)src, (short*)out,
                                        scheme);
  return hipGetLastError();
}
