// fp32 MFMA weight gradient for the square, K-split case: lin_l's dW = dh^T x after the source gather
// (M = N = 512 features, K = 20000 node rows in 16 splits), the one launch the whole chip waits on.
//
//   slab[z][M][N] = A[kb..ke, M]^T B[kb..ke, N],  kb = z * kchunk, ke = min(K, kb + kchunk);
//   A = dY [K, M] and B = X [K, N], both K-major (row-major over node rows); the caller's split-order
//   slab sum (reduce.hip colsum_wide4) finishes dW.
//
// Reference: the lin_l weight gradient of PyG GATConv (models.py:619), ATen/MKL sgemm on the CPU.
//
// Same tile and arithmetic as gemm_kernel<128, 128, true, true, ...> of gemm.hip (128 x 128 output
// tile, 4 waves in 2 x 2, each a 64 x 64 wave tile of v_mfma_f32_32x32x2_f32), but that kernel runs
// here at one workgroup per CU = one wave per SIMD and stages every 16-deep K-step global -> VGPR ->
// LDS between two barriers with nothing to cover the round trip.  This one feeds the same MFMAs
// through the LDS-DMA ring of gemm_tall.hip:
//  * K in 16-deep stages, both operands as [k][128] rows (8 KiB each), a 3-slot ring = 48 KiB static
//    LDS; stage s+2 is copied by global_load_lds_dwordx4 while stage s is multiplied: one raw barrier
//    per stage, a counted vmcnt, no VGPR staging.  A wave's four 1-KiB pieces of a stage are issued
//    one per second MFMA group, each between two MFMAs of the group (a piece costs ~60 issue cycles:
//    all four at the barrier, or one in front of a group, leave the matrix pipe idle);
//  * k rows past the split's end (the ragged last stage) are copied from a zero row: LDS-DMA has no
//    per-lane fill value, and a lane switched off would change the vmcnt count.  The two stages
//    issued past the last one copy the zero row as well, into slots nobody reads any more;
//  * fragments are ds_read_b32 of 32 consecutive floats of k row 2g + (lane >> 5) (conflict-free: the
//    two half-waves are separate LDS lane groups), read one MFMA group ahead into a second register
//    set and waited for by a counted lgkmcnt, so with one wave per SIMD the matrix pipe does not
//    drain at an LDS round trip; the stage's last group is multiplied after the next stage's barrier
//    and first read;
//  * the reads are inline asm for the reason given in gemm_tall.hip (the compiler cannot tell ring
//    slots apart and would drain the copies in flight before every LDS read);
//  * the 16 splits x 16 tiles are placed so that an XCD holds whole splits: each A and B stage is
//    fetched into one L2 and shared by the four tiles that use it.
// Summation order: every output element accumulates its split's k in ascending order, two per MFMA
// (lane >> 5 picks the k of the pair), in the same stages with the same zero padding as gemm_tile,
// so the slabs are bit-identical to the old kernel's on every input.
// No bias-gradient column sums (gemm_tile's CS form): lin_l has no Linear bias.  Callers that want
// db with dW (hicgat_gemm_wgrad, the grouped launch) keep gemm_tile.
#include "common.hpp"

namespace hicgat {

namespace {

constexpr int WBM = 128, WBN = 128, WBK = 16, WSLOTS = 3;
constexpr int WOP_F = WBM * WBK;        // floats of one operand's stage: [16][128] (8 KiB)
constexpr int WSTAGE_F = 2 * WOP_F;     // A rows, then B rows (16 KiB)
constexpr int WPIECES = 4;              // 1-KiB LDS-DMA pieces per wave and stage (2 of A, 2 of B)

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ const float wgrad_zero_row[WBM] = {};

// One 1-KiB LDS-DMA piece: lane l's 16 bytes at src land at LDS byte address dst + 16 l (dst wave-uniform).
// Inline asm, so that the piece can be placed between two MFMAs and is not preceded by the
// s_waitcnt lgkmcnt(0) the compiler puts in front of the builtin (it would expose the fragment reads
// just issued); M0 is the compiler's and is put back in the same statement.
__device__ __forceinline__ void wgrad_glds(const float *src, uint32_t dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(dst)
               : "memory");
}

}  // namespace

__global__ __launch_bounds__(256, 2) void gemm_wgrad_ring_kernel(const float *__restrict__ A, int64_t lda,
                                                                const float *__restrict__ B, int64_t ldb, int M,
                                                                int N, int K, int kchunk, float *__restrict__ slab,
                                                                int64_t slab_stride) {
  __shared__ __attribute__((aligned(16))) float lds[WSLOTS * WSTAGE_F];
  const int lane = threadIdx.x & 63, w = wave_in_block();
  const int li = lane & 31, lk = lane >> 5;
  const int wm = w >> 1, wn = w & 1;
  // XCD-aware: consecutive (tile, split) ids on one XCD, tiles of a split together
  const int tm = M / WBM, per = tm * (N / WBN);
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int bz = id / per, rem = id - bz * per;
  const int m0 = (rem % tm) * WBM, n0 = (rem / tm) * WBN;
  const int kb = bz * kchunk, ke = min(K, kb + kchunk);
  const int S = kb < ke ? (ke - kb + WBK - 1) / WBK : 0;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  // This wave's share of a stage: four 1-KiB pieces, k rows 2p, 2p + 1 (p = w and w + 4) of A and of B;
  // lane -> k row 2p + lane / 32, columns 4 * (lane % 32) .. + 3.  gk / pa / pb walk down the split one
  // stage (16 rows) per issue; a row at or past ke is copied from the zero row instead (so is every
  // piece of the two stages issued past the last one: the count of copies per stage never changes,
  // and one vmcnt serves every stage).
  const uint32_t lds_base = (uint32_t)(uintptr_t)lds;
  const int c4 = (lane & 31) * 4;
  const float *zr = wgrad_zero_row + c4;
  int gk[2];
  const float *pa[2], *pb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    gk[h] = kb + 2 * (w + 4 * h) + (lane >> 5);
    pa[h] = A + (size_t)gk[h] * lda + m0 + c4;
    pb[h] = B + (size_t)gk[h] * ldb + n0 + c4;
  }
  auto piece_src = [&](int q) { return gk[q >> 1] < ke ? ((q & 1) ? pb[q >> 1] : pa[q >> 1]) : zr; };
  auto piece_dst = [&](int slot_, int q) {
    return lds_base + (uint32_t)((slot_ * WSTAGE_F + (q & 1) * WOP_F + (w + 4 * (q >> 1)) * 256) * 4);
  };
  auto advance = [&](int h) {
    gk[h] += WBK;
    pa[h] += (size_t)WBK * lda;
    pb[h] += (size_t)WBK * ldb;
  };
#pragma unroll
  for (int st = 0; st < 2; ++st) {   // stages 0 and 1
#pragma unroll
    for (int q = 0; q < WPIECES; ++q) wgrad_glds(piece_src(q), piece_dst(st, q));
    advance(0);
    advance(1);
  }

  // per-lane LDS byte offsets of the fragments inside a stage: k row lk, columns of the wave tile
  const uint32_t a_off = (uint32_t)((lk * WBM + wm * 64 + li) * 4);
  const uint32_t b_off = (uint32_t)((WOP_F + lk * WBN + wn * 64 + li) * 4);

  // f[g & 1]: the fragments of MFMA group g (k rows 2g, 2g + 1): a0, a1 (rows +0, +32), b0, b1.
  // f[1] enters a stage holding the previous stage's group 7 (zeros before the first: 0 * 0 + 0).
  float f[2][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) f[1][i] = 0.f;
  auto mfma = [&](const float (&v)[4], int a, int b) {
    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[a], v[2 + b], acc[a][b], 0, 0, 0);
  };
  auto mma = [&](const float (&v)[4]) {
    mfma(v, 0, 0);
    mfma(v, 0, 1);
    mfma(v, 1, 0);
    mfma(v, 1, 1);
  };

  int slot = 0;   // s % WSLOTS
  for (int s = 0; s < S; ++s) {
    // this wave's copy of stage s has landed (the four pieces of stage s+1 may stay in flight)
    asm volatile("s_waitcnt vmcnt(4)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();   // every wave's copy landed; every wave is past stage s-1's reads
    asm volatile("" ::: "memory");
    const uint32_t st = lds_base + (uint32_t)(slot * WSTAGE_F * 4);
    const uint32_t aa = st + a_off, ba = st + b_off;
    const int nslot = slot == 0 ? WSLOTS - 1 : slot - 1;   // (s + 2) % WSLOTS: stage s-1's, free now

    asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:128\n\t"
                 "ds_read_b32 %2, %5\n\tds_read_b32 %3, %5 offset:128"
                 : "=&v"(f[0][0]), "=&v"(f[0][1]), "=&v"(f[0][2]), "=&v"(f[0][3])
                 : "v"(aa), "v"(ba)
                 : "memory");
    __builtin_amdgcn_sched_barrier(0);
    mma(f[1]);   // group 7 of stage s-1, behind the barrier and the first reads: it covers their latency
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < WBK / 2; ++g) {
      float(&cur)[4] = f[g & 1];
      float(&nxt)[4] = f[(g + 1) & 1];
      if (g + 1 < WBK / 2) {
        // group g+1's reads go out, then group g's (the four before them) are waited for
        const uint32_t an = aa + (uint32_t)((g + 1) * 2 * WBM * 4), bn = ba + (uint32_t)((g + 1) * 2 * WBN * 4);
        asm volatile("ds_read_b32 %0, %8\n\tds_read_b32 %1, %8 offset:128\n\t"
                     "ds_read_b32 %2, %9\n\tds_read_b32 %3, %9 offset:128\n\t"
                     "s_waitcnt lgkmcnt(4)"
                     : "=&v"(nxt[0]), "=&v"(nxt[1]), "=&v"(nxt[2]), "=&v"(nxt[3]), "+v"(cur[0]), "+v"(cur[1]),
                       "+v"(cur[2]), "+v"(cur[3])
                     : "v"(an), "v"(bn)
                     : "memory");
        if (g & 1) {
          mma(cur);
        } else {
          // piece g / 2 of stage s+2 inside this group: its address behind the first MFMA, the copy
          // behind the second -- each fits the issue slots an executing MFMA leaves free
          const int q = g >> 1;
          mfma(cur, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          const float *src = piece_src(q);
          asm volatile("" : "+v"(src));
          if (q & 1) advance(q >> 1);
          __builtin_amdgcn_sched_barrier(0);
          mfma(cur, 0, 1);
          __builtin_amdgcn_sched_barrier(0);
          wgrad_glds(src, piece_dst(nslot, q));
          __builtin_amdgcn_sched_barrier(0);
          mfma(cur, 1, 0);
          mfma(cur, 1, 1);
        }
      } else {
        // the stage's last reads have landed: the next barrier may free the slot; their MFMAs follow it
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cur[0]), "+v"(cur[1]), "+v"(cur[2]), "+v"(cur[3])::"memory");
      }
    }
    slot = slot == WSLOTS - 1 ? 0 : slot + 1;
  }
  mma(f[1]);   // group 7 of the last stage (zeros for an empty split)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the copies issued past the last stage

  // C/D map of a 32x32 f32 tile: col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float *out = slab + (size_t)bz * slab_stride;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int gn = n0 + wn * 64 + b * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        out[(size_t)gm * N + gn] = acc[a][b][r];
      }
    }
}

// The ring kernel takes the problem when it fits its tiling (the caller has checked splits > 1 and the
// slab): returns HICGAT_EUNSUPPORTED otherwise, and the caller uses gemm_kernel<128, 128, ...>.
// Whether a K-split weight gradient fits the ring kernel's tiling (whole 128 x 128 tiles up to 1024,
// rows and operands the 16-byte LDS-DMA copies can read): the one statement of it, asked by the
// dispatch of gemm.hip (and its hicgat_gemm_form) and by the launch below.  Addresses: alignment only.
bool gemm_wgrad_ring_fits(const void *A, int64_t lda, const void *B, int64_t ldb, int M, int N, int K, int splits) {
  const bool al = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0;
  if (!al || M % WBM || N % WBN || M < WBM || N < WBN || M > 1024 || N > 1024 || lda % 4 || ldb % 4 || K < 1)
    return false;
  return (int64_t)(M / WBM) * (N / WBN) * splits <= 0x7fffffff;
}

int gemm_wgrad_ring_launch(const float *A, int64_t lda, const float *B, int64_t ldb, int M, int N, int K, int kchunk,
                           int splits, float *slab, int64_t slab_stride, hipStream_t s) {
  // kchunk: the caller's split depth, whole 16-deep stages (launch<> of gemm.hip rounds it so)
  if (!gemm_wgrad_ring_fits(A, lda, B, ldb, M, N, K, splits) || kchunk % WBK) return HICGAT_EUNSUPPORTED;
  const int64_t wgs = (int64_t)(M / WBM) * (N / WBN) * splits;
  hipLaunchKernelGGL(gemm_wgrad_ring_kernel, dim3((unsigned)wgs), dim3(256), 0, s, A, lda, B, ldb, M, N, K, kchunk,
                     slab, slab_stride);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

}  // namespace hicgat
