// All-pairs 3-D distance, MSE + Pearson moments and their gradient on gfx950 (a7, a8, a9).
//
// Reference: out = torch.cdist(c, c, p=2) (models.py:661) -> MSELoss()(out, truth)
// (HiC-GNN_main.py:127), scipy pearsonr of the triu pairs (HiC_GAT_generalize_directly.py:220), and
// the contrastive loss 0.1 * mean_{i<j} |T_ij - D_ij| (train_and_test_same_res_GAT_node2vec.py:107-134).
// The reference materialises D [N, N] (and its grad) in HBM; the fused kernel here streams the
// truth matrix once, only its upper-triangle 128x128 tiles, and never stores D.
//
// Tile kernel: one 256-thread block per 128x128 tile; thread (ty, tx) in a 16x16 grid owns rows
// {4ty..4ty+3, 64+4ty..} x cols {4tx..4tx+3, 64+4tx..}, so every T row segment is two coalesced
// 256 B float4 sweeps.  Per pair it forms d, r = d - t, the moments and w = r/d, and accumulates
// w*(c_i - c_j) into row partials (reduced over the 16 tx lanes) and column partials (reduced over
// ty through LDS).  Partials go to a [tile][2][128] float4 slab and a second kernel adds, per row,
// the slabs of every tile touching it in a fixed order: bitwise reproducible, no float atomics.
//
// Two chains share everything around the per-pair arithmetic (stage_coords, col_partials / col_sums /
// row_sums, the moment records, gather_row, moments_partial_block, moment_stats, PdLayout): the
// fixed-weight chain (MSE, combined, contrastive: 3 float planes, 7 moments, 2 slabs per tile) and the
// moment-dependent chain (mloss: 6 planes, 8 moments, 4 slabs per tile).
#include <algorithm>
#include <type_traits>
#include <cstdint>
#include <cstdlib>

#include "common.hpp"

namespace hicgat {

constexpr int BT = 128;
enum { MODE_SYM = 0, MODE_FULL = 1 };
// loss kinds (include/hicgat.h): the KIND template parameter below
enum { KIND_MSE = HICGAT_LOSS_MSE, KIND_COMBINED = HICGAT_LOSS_COMBINED, KIND_CONTRASTIVE = HICGAT_LOSS_CONTRASTIVE };

// d|r|/dr = sign(r) with sign(0) = 0 (torch.abs's backward, sgn), times inv = 1/d
__device__ __forceinline__ float sgn_inv(float r, float inv) { return r == 0.f ? 0.f : copysignf(inv, r); }

__host__ __device__ inline int pd_nb(int N) { return (N + BT - 1) / BT; }
__host__ __device__ inline int64_t tri_start(int64_t I, int64_t nb) { return I * nb - I * (I - 1) / 2; }

__device__ inline void tri_decode(int64_t t, int nb, int &I, int &J) {
  const double b = 2.0 * nb + 1.0;
  int64_t Ii = (int64_t)floor((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (Ii < 0) Ii = 0;
  if (Ii > nb - 1) Ii = nb - 1;
  while (Ii > 0 && tri_start(Ii, nb) > t) --Ii;
  while (Ii + 1 < nb && tri_start(Ii + 1, nb) <= t) ++Ii;
  // block-uniform: into SGPRs, so every branch on I / J (interior vs edge tiles) is a scalar
  // branch, not an if-converted (both paths) VALU select
  I = __builtin_amdgcn_readfirstlane((int)Ii);
  J = __builtin_amdgcn_readfirstlane((int)(Ii + (t - tri_start(Ii, nb))));
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Sum over the 16 lanes of a DPP row (the 16 tx lanes sharing ty): row rotations by 8 and 4, then
// quad permutes (xor 2, xor 1); VALU-only, every lane ends with the row sum.
__device__ __forceinline__ float sum16(float v) {
  v += dpp<0x128>(v);   // row_ror:8
  v += dpp<0x124>(v);   // row_ror:4
  v += dpp<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp<0xB1>(v);    // quad_perm [1,0,3,2]
  return v;
}


// v + the values of lanes l^16, l^32 and l^48 (ds_bpermute shuffles; a v_permlane16/32_swap form
// measured slower: the loss chain 0.162 vs 0.157 ms, profiles/r04h_kbench_pairdist.txt)
__device__ __forceinline__ float sum_rows4(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

__device__ __forceinline__ double shfl_xor_d(double v, int m) {
  const int2 p = *reinterpret_cast<int2 *>(&v);
  int2 q;
  q.x = __shfl_xor(p.x, m);
  q.y = __shfl_xor(p.y, m);
  return *reinterpret_cast<double *>(&q);
}

__device__ __forceinline__ void add3(float4 &s, const float4 &o) { s.x += o.x; s.y += o.y; s.z += o.z; }

// A 256-thread block's moment record, M doubles: the components of MASK summed over the wave (the
// others are taken from lane 0 as they are: the callers leave those at 0) into mred[wave]; after a
// barrier, moment_record adds the 4 waves in the fixed order ((0 + 1) + 2) + 3.
template <int M, unsigned MASK = (1u << M) - 1>
__device__ __forceinline__ void moment_wave_sums(double (&m)[M], double (*mred)[M], int lane, int wv) {
#pragma unroll
  for (int c = 0; c < M; ++c) {
    if (!((MASK >> c) & 1)) continue;
    for (int o = 32; o > 0; o >>= 1) m[c] += shfl_xor_d(m[c], o);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < M; ++c) mred[wv][c] = m[c];
  }
}

template <int M>
__device__ __forceinline__ void moment_record(const double (*mred)[M], double *__restrict__ rec) {
  const int c = threadIdx.x;
  if (c < M) rec[c] = ((mred[0][c] + mred[1][c]) + mred[2][c]) + mred[3][c];
}

// Row partials of the background form: each thread's 8-column partial of every row it touches goes
// to LDS and threads 128..255 add the 16 per row in tx order at the end, while 0..127 add the column
// partials -- instead of three 16-lane DPP sums per row inside the pair loop (~20 % of its VALU
// issue).  Three planes (x, y, z) of [128 rows][kRowPad] floats, 30 KB where float4 entries took 34:
// with the planar colred the workgroup holds 39.4 KB of LDS, four per CU.  kRowPad = 20: a 32-lane
// half's ds_write_b32 (two ty, rows 4 apart = 80 dwords = 16 banks) is conflict-free, and the row
// sums read their 16 floats as four conflict-free ds_read_b128 (80-B rows: 16 lanes, 16 slots).
constexpr int kRowPad = 20;
constexpr int kRowPlane = BT * kRowPad;

// ---- per-pair bodies ------------------------------------------------------------------------------

// Per-thread accumulators of one tile: the moments and the column partials of its 8 columns.
struct TileAcc {
  float L = 0.f, sd = 0.f, sdd = 0.f, sdt = 0.f, st = 0.f, stt = 0.f, dg = 0.f;
  float ax[8], ay[8], az[8];
};

// The 8 rows x 8 columns of one thread.  MASK: the diagonal and the edge tiles (row / column
// bounds, i < j on the diagonal, the diagonal moment); interior tiles take MASK = false and do
// no per-pair selection at all.  d2 == 0 (coincident points) gives inv = 1e30, d = 0 and a finite
// w times dx = dy = dz = 0, i.e. no gradient -- torch's _euclidean_dist_backward masks it too.
template <int MODE, bool VEC, int KIND, bool MASK, int K0, int K1, bool BG = false, bool RLDS = false>
__device__ __forceinline__ void tile_rows(const float *__restrict__ T, int64_t ldt, int64_t row0, int64_t col0,
                                          int N, int I, int J, float bg,
                                          const float *tile, const float (*sc)[BT][3], int tx, int ty,
                                          const float *cx, const float *cy, const float *cz, int gj0,
                                          float4 *__restrict__ prow, TileAcc &A, float *rowpart) {
  constexpr bool PEARSON = KIND == KIND_COMBINED, ABSL = KIND == KIND_CONTRASTIVE;
#pragma unroll 1
  for (int k = K0; k < K1; ++k) {
    const int lr = ty * 4 + (k & 3) + (k >> 2) * 64;
    const int gi = I * BT + lr;
    const float rx = sc[0][lr][0], ry = sc[0][lr][1], rz = sc[0][lr][2];
    // the thread's global columns from one base (gj0 + 0..3, gj0 + 64..67): one register, not eight
    int gj[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) gj[q] = gj0 + (q & 3) + (q >> 2) * 64;
    float tv[8];
    if (BG) {   // background form: every pair at the background value, the support added later
#pragma unroll
      for (int q = 0; q < 8; ++q) tv[q] = bg;
    } else if (VEC) {  // from the LDS image of the tile (conflict-free ds_read_b128: 16 lanes = one row)
      const float4 a = *reinterpret_cast<const float4 *>(&tile[lr * BT + tx * 4]);
      const float4 b = *reinterpret_cast<const float4 *>(&tile[lr * BT + 64 + tx * 4]);
      tv[0] = a.x; tv[1] = a.y; tv[2] = a.z; tv[3] = a.w;
      tv[4] = b.x; tv[5] = b.y; tv[6] = b.z; tv[7] = b.w;
    } else if (gi < N) {
      const float *trow = T + (size_t)(gi - row0) * ldt + (size_t)((int64_t)J * BT - col0);
#pragma unroll
      for (int q = 0; q < 8; ++q) tv[q] = gj[q] < N ? trow[tx * 4 + (q & 3) + (q >> 2) * 64] : 0.f;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) tv[q] = 0.f;
    }
    float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float dx = rx - cx[q], dy = ry - cy[q], dz = rz - cz[q];
      const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
      // one v_rsq for both d and 1/d (1-2 ulp; the reference's own mm-formula cdist is far
      // coarser)
      const float inv = fminf(__builtin_amdgcn_rsqf(d2), 1e30f);
      const float d = d2 * inv;
      const float tt = tv[q];
      float w;
      if (MODE == MODE_SYM) {
        const float r = d - tt;
        if (MASK) {
          bool valid = gi < N && gj[q] < N;
          // (D_ii - T_ii)^2 = T_ii^2 (MSE over all N^2 entries; the contrastive loss is over i < j only)
          if (!BG && !ABSL && valid && gi == gj[q]) A.dg = fmaf(tt, tt, A.dg);
          valid = valid && (I != J || gi < gj[q]);
          if (valid) {
            A.L = ABSL ? A.L + fabsf(r) : fmaf(r, r, A.L);
            if (PEARSON) {
              A.sd += d;
              A.sdd = fmaf(d, d, A.sdd);
              A.sdt = fmaf(d, tt, A.sdt);
              A.st += tt;
              A.stt = fmaf(tt, tt, A.stt);
            }
          }
          w = valid ? (ABSL ? sgn_inv(r, inv) : r * inv) : 0.f;
        } else {
          A.L = ABSL ? A.L + fabsf(r) : fmaf(r, r, A.L);
          if (PEARSON) {
            A.sd += d;
            A.sdd = fmaf(d, d, A.sdd);
            A.sdt = fmaf(d, tt, A.sdt);
            A.st += tt;
            A.stt = fmaf(tt, tt, A.stt);
          }
          w = ABSL ? sgn_inv(r, inv) : r * inv;
        }
      } else {
        w = tt * inv;
        if (MASK) w = (gi < N && gj[q] < N && gi != gj[q]) ? w : 0.f;
      }
      px = fmaf(w, dx, px);
      py = fmaf(w, dy, py);
      pz = fmaf(w, dz, pz);
      A.ax[q] = fmaf(-w, dx, A.ax[q]);
      A.ay[q] = fmaf(-w, dy, A.ay[q]);
      A.az[q] = fmaf(-w, dz, A.az[q]);
    }
    if constexpr (RLDS) {   // the thread's 8-column partial of row lr; the 16 of a row are added at the end
      rowpart[lr * kRowPad + tx] = px;
      rowpart[kRowPlane + lr * kRowPad + tx] = py;
      rowpart[2 * kRowPlane + lr * kRowPad + tx] = pz;
    } else {
      px = sum16(px);
      py = sum16(py);
      pz = sum16(pz);
      if (tx == 0) prow[lr] = make_float4(px, py, pz, 0.f);
    }
  }
}

// Interior tiles of the training loss (MODE_SYM, T from the LDS image, no masks) in packed fp32:
// the thread's 8 columns as 4 float2 pairs, so the subtractions, multiplies and FMAs issue as
// v_pk_{add,mul,fma}_f32 (two pairs per instruction); v_rsq stays scalar.
typedef float f2 __attribute__((ext_vector_type(2)));

template <int KIND, int K0, int K1, bool BG = false, bool RLDS = false>
__device__ __forceinline__ void tile_rows_pk(const float *tile, float bg, const float (*sc)[BT][3], int tx, int ty,
                                             const float *cx, const float *cy, const float *cz,
                                             float4 *__restrict__ prow, TileAcc &A, float *rowpart) {
  constexpr bool PEARSON = KIND == KIND_COMBINED, ABSL = KIND == KIND_CONTRASTIVE;
  f2 cx2[4], cy2[4], cz2[4], ax2[4], ay2[4], az2[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    cx2[h] = f2{cx[2 * h], cx[2 * h + 1]};
    cy2[h] = f2{cy[2 * h], cy[2 * h + 1]};
    cz2[h] = f2{cz[2 * h], cz[2 * h + 1]};
    ax2[h] = f2{A.ax[2 * h], A.ax[2 * h + 1]};
    ay2[h] = f2{A.ay[2 * h], A.ay[2 * h + 1]};
    az2[h] = f2{A.az[2 * h], A.az[2 * h + 1]};
  }
  const f2 z2 = f2{0.f, 0.f};
  f2 L2 = z2, sd2 = z2, sdd2 = z2, sdt2 = z2, st2 = z2, stt2 = z2;
#pragma unroll 2   // rows per iteration (the next row's LDS reads in flight)
  for (int k = K0; k < K1; ++k) {
    const int lr = ty * 4 + (k & 3) + (k >> 2) * 64;
    const f2 rx = f2{sc[0][lr][0], sc[0][lr][0]}, ry = f2{sc[0][lr][1], sc[0][lr][1]},
             rz = f2{sc[0][lr][2], sc[0][lr][2]};
    f2 tv[4];
    if constexpr (BG) {
#pragma unroll
      for (int h = 0; h < 4; ++h) tv[h] = f2{bg, bg};
    } else {
      const float4 a = *reinterpret_cast<const float4 *>(&tile[lr * BT + tx * 4]);
      const float4 b = *reinterpret_cast<const float4 *>(&tile[lr * BT + 64 + tx * 4]);
      tv[0] = f2{a.x, a.y};
      tv[1] = f2{a.z, a.w};
      tv[2] = f2{b.x, b.y};
      tv[3] = f2{b.z, b.w};
    }
    f2 px = z2, py = z2, pz = z2;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const f2 dx = rx - cx2[h], dy = ry - cy2[h], dz = rz - cz2[h];
      // d2 + 2^-100 (below one ulp of any d2 that is not ~0): coincident points give a finite
      // inv = 2^50, d = 2^-50 and w * (dx, dy, dz) = 0 -- the clamp of the generic path for free
      const f2 d2 = __builtin_elementwise_fma(dx, dx, __builtin_elementwise_fma(dy, dy,
                                              __builtin_elementwise_fma(dz, dz, f2{0x1.0p-100f, 0x1.0p-100f})));
      const f2 inv = f2{__builtin_amdgcn_rsqf(d2.x), __builtin_amdgcn_rsqf(d2.y)};
      const f2 d = d2 * inv;
      const f2 r = d - tv[h];
      if constexpr (ABSL) L2 += __builtin_elementwise_abs(r);
      else L2 = __builtin_elementwise_fma(r, r, L2);
      if (PEARSON) {
        sd2 += d;
        sdd2 = __builtin_elementwise_fma(d, d, sdd2);
        if constexpr (!BG) {   // background form: t = bg at every pair, these three follow below
          sdt2 = __builtin_elementwise_fma(d, tv[h], sdt2);
          st2 += tv[h];
          stt2 = __builtin_elementwise_fma(tv[h], tv[h], stt2);
        }
      }
      const f2 w = ABSL ? f2{sgn_inv(r.x, inv.x), sgn_inv(r.y, inv.y)} : r * inv;
      px = __builtin_elementwise_fma(w, dx, px);
      py = __builtin_elementwise_fma(w, dy, py);
      pz = __builtin_elementwise_fma(w, dz, pz);
      ax2[h] = __builtin_elementwise_fma(-w, dx, ax2[h]);
      ay2[h] = __builtin_elementwise_fma(-w, dy, ay2[h]);
      az2[h] = __builtin_elementwise_fma(-w, dz, az2[h]);
    }
    if constexpr (RLDS) {
      rowpart[lr * kRowPad + tx] = px.x + px.y;
      rowpart[kRowPlane + lr * kRowPad + tx] = py.x + py.y;
      rowpart[2 * kRowPlane + lr * kRowPad + tx] = pz.x + pz.y;
    } else {
      const float sx = sum16(px.x + px.y), sy = sum16(py.x + py.y), sz = sum16(pz.x + pz.y);
      if (tx == 0) prow[lr] = make_float4(sx, sy, sz, 0.f);
    }
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    A.ax[2 * h] = ax2[h].x;
    A.ax[2 * h + 1] = ax2[h].y;
    A.ay[2 * h] = ay2[h].x;
    A.ay[2 * h + 1] = ay2[h].y;
    A.az[2 * h] = az2[h].x;
    A.az[2 * h + 1] = az2[h].y;
  }
  const float L = L2.x + L2.y;
  A.L += L;
  if (PEARSON) {
    const float sd = sd2.x + sd2.y;
    A.sd += sd;
    A.sdd += sdd2.x + sdd2.y;   // summed directly in every form: sum (d - bg)^2 + bg (2 sum d - n bg)
                                // cancels when d << bg (collapsed coordinates early in training)
    if constexpr (BG) {
      // t = bg at all 8 (K1 - K0) pairs: sum d t = bg sum d, sum t and sum t^2 by count (three packed
      // ops per two pairs out of the loop)
      constexpr float npair = 8.f * (K1 - K0);
      A.sdt = fmaf(bg, sd, A.sdt);
      A.st = fmaf(npair, bg, A.st);
      A.stt = fmaf(npair * bg, bg, A.stt);
    } else {
      A.sdt += sdt2.x + sdt2.y;
      A.st += st2.x + st2.y;
      A.stt += stt2.x + stt2.y;
    }
  }
}

// ---- moment-dependent losses (mse + alpha (1 - r), rmse, scale-invariant mse) ---------------------
// Their derivative per pair is g_ij = A d_ij + B t_ij + C with A, B, C functions of the global
// moments, which are only known after the pass.  With u_ij = (c_i - c_j) / d_ij (0 where d_ij = 0):
//   dc_i = sum_j g_ij u_ij = -B R_i + (A + B) U_i + C W_i,
//   R_i = sum_j (d_ij - t_ij) u_ij,  U_i = sum_j (c_i - c_j) = N c_i - sum_j c_j,  W_i = sum_j u_ij,
// so one tile pass accumulates R and W (and all the moments) without A, B, C; a per-row combine
// applies them in fp64 after the moments are final (mloss_finalize_kernel).
enum { MLOSS_PEARSON = HICGAT_MLOSS_PEARSON, MLOSS_RMSE = HICGAT_MLOSS_RMSE, MLOSS_SI_MSE = HICGAT_MLOSS_SI_MSE };

constexpr int kMPlanes = 6;   // row partial planes in LDS: R x/y/z, W x/y/z
constexpr double kVarFloor = 0x1.0p-20;   // see mloss_finalize_kernel

// Per-thread accumulators of one tile, packed: the column partials of R and W for the thread's 8
// columns (4 float2 each) and the six pair moments.
struct MTileAcc {
  f2 ax[4], ay[4], az[4], bx[4], by[4], bz[4];
  f2 L, sd, sdd, sdt, st, stt;
  double dg = 0.0, sg = 0.0;   // sum T_ii^2, sum T_ii (diagonal tiles of the dense form), exact products:
                               // si_mse subtracts the squared mean from them
};

// The thread's 8 rows x 8 columns in packed fp32.  MASK (diagonal and edge tiles): pairs outside
// i < j < N get t = 0 and d, 1/d scaled by 0, so every sum below leaves them out with no select in
// the arithmetic.  d^2 == 0 (coincident points): inv = 2^50 and d = 0 exactly, dx = dy = dz = 0, so
// neither R nor W gets a term -- u_ij = 0 there.  BG: t = bg at every pair, no T read.
template <bool MASK, bool BG>
__device__ __forceinline__ void mloss_rows(const float *__restrict__ T, int64_t ldt, bool vec, int N, int I, int J,
                                           float bg, const float (*sc)[BT][3], int tx, int ty, const f2 *cx2,
                                           const f2 *cy2, const f2 *cz2, int gj0, MTileAcc &A, float *rowpart) {
  const f2 z2 = f2{0.f, 0.f}, eps2 = f2{0x1.0p-100f, 0x1.0p-100f};
#pragma unroll 2
  for (int k = 0; k < 8; ++k) {
    const int lr = ty * 4 + (k & 3) + (k >> 2) * 64;
    const int gi = I * BT + lr;
    const f2 rx = f2{sc[0][lr][0], sc[0][lr][0]}, ry = f2{sc[0][lr][1], sc[0][lr][1]},
             rz = f2{sc[0][lr][2], sc[0][lr][2]};
    float tv[8];
    if constexpr (BG) {
#pragma unroll
      for (int q = 0; q < 8; ++q) tv[q] = bg;
    } else if (vec) {   // block-uniform: two 16-B loads (a 16-lane row sweeps 256 B); rows past N clamped, masked below
      const float *trow = T + (size_t)min(gi, N - 1) * ldt + (size_t)J * BT + tx * 4;
      const float4 a = *reinterpret_cast<const float4 *>(trow);
      const float4 b = *reinterpret_cast<const float4 *>(trow + 64);
      tv[0] = a.x; tv[1] = a.y; tv[2] = a.z; tv[3] = a.w;
      tv[4] = b.x; tv[5] = b.y; tv[6] = b.z; tv[7] = b.w;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int gj = gj0 + (q & 3) + (q >> 2) * 64;
        tv[q] = (gi < N && gj < N) ? T[(size_t)gi * ldt + gj] : 0.f;
      }
    }
    float mk[8];
    if constexpr (MASK) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int gj = gj0 + (q & 3) + (q >> 2) * 64;
        const bool in = gi < N && gj < N;
        if (!BG && in && gi == gj) {   // the diagonal entry: (0 - T_ii)^2 of the all-entries mean, and T_ii
          A.dg += (double)tv[q] * (double)tv[q];
          A.sg += (double)tv[q];
        }
        const bool valid = in && (I != J || gi < gj);
        mk[q] = valid ? 1.f : 0.f;
        tv[q] = valid ? tv[q] : 0.f;
      }
    }
    f2 px = z2, py = z2, pz = z2, qx = z2, qy = z2, qz = z2;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const f2 dx = rx - cx2[h], dy = ry - cy2[h], dz = rz - cz2[h];
      const f2 d2 = __builtin_elementwise_fma(dx, dx, __builtin_elementwise_fma(dy, dy, dz * dz));
      const f2 d2e = d2 + eps2;
      f2 inv = f2{__builtin_amdgcn_rsqf(d2e.x), __builtin_amdgcn_rsqf(d2e.y)};
      if constexpr (MASK) inv *= f2{mk[2 * h], mk[2 * h + 1]};
      const f2 d = d2 * inv;
      const f2 t = f2{tv[2 * h], tv[2 * h + 1]};
      const f2 r = d - t;
      A.L = __builtin_elementwise_fma(r, r, A.L);
      A.sd += d;
      A.sdd = __builtin_elementwise_fma(d, d, A.sdd);
      if constexpr (!BG || MASK) {   // BG interior: t = bg at all 64 pairs, these three by count below
        A.sdt = __builtin_elementwise_fma(d, t, A.sdt);
        A.st += t;
        A.stt = __builtin_elementwise_fma(t, t, A.stt);
      }
      const f2 w = r * inv;
      px = __builtin_elementwise_fma(w, dx, px);
      py = __builtin_elementwise_fma(w, dy, py);
      pz = __builtin_elementwise_fma(w, dz, pz);
      A.ax[h] = __builtin_elementwise_fma(-w, dx, A.ax[h]);
      A.ay[h] = __builtin_elementwise_fma(-w, dy, A.ay[h]);
      A.az[h] = __builtin_elementwise_fma(-w, dz, A.az[h]);
      qx = __builtin_elementwise_fma(inv, dx, qx);
      qy = __builtin_elementwise_fma(inv, dy, qy);
      qz = __builtin_elementwise_fma(inv, dz, qz);
      A.bx[h] = __builtin_elementwise_fma(-inv, dx, A.bx[h]);
      A.by[h] = __builtin_elementwise_fma(-inv, dy, A.by[h]);
      A.bz[h] = __builtin_elementwise_fma(-inv, dz, A.bz[h]);
    }
    // the thread's 8-column partial of row lr; the 16 of a row are added in tx order at the end
    float *rp = rowpart + lr * kRowPad + tx;
    rp[0] = px.x + px.y;
    rp[kRowPlane] = py.x + py.y;
    rp[2 * kRowPlane] = pz.x + pz.y;
    rp[3 * kRowPlane] = qx.x + qx.y;
    rp[4 * kRowPlane] = qy.x + qy.y;
    rp[5 * kRowPlane] = qz.x + qz.y;
  }
}

// Support pass of the background form: T = bg except at the sorted CSR support (symmetric, no
// diagonal) and the diagonal.  One wave per row i, lanes over its support entries j:
//   gradient  corr[i] = sum_j ((d - t) - (d - bg)) / d * (c_i - c_j) = sum_j (bg - t) / d * (c_i - c_j)
//             (every j: the bulk tiles gave row i the bg term of each pair, as row or column partial);
//   moments   over j > i only (each pair once, in fp64), the support's change of the bulk's terms:
//             L += (d - t)^2 - (d - bg)^2, sdt += d (t - bg), st += t - bg, stt += t^2 - bg^2; and the
//             diagonal's (0 - T_ii)^2 into the dg moment.
// Contrastive (KIND_CONTRASTIVE): corr[i] = sum_j (sgn(d - t) - sgn(d - bg)) / d * (c_i - c_j), and
// L += |d - t| - |d - bg| over j > i; no diagonal term (the loss is over i < j only).
// d is formed exactly as in the bulk's interior path.  Per-block moment records (fixed order).
template <int KIND>
__device__ void support_block(const float *__restrict__ coords, float bg, int row_begin, int row_end,
                              const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                              const float *__restrict__ val, const float *__restrict__ diag, float4 *__restrict__ corr,
                              double *__restrict__ mom, const int *__restrict__ cmap, int blk,
                              const float4 *__restrict__ cpad = nullptr) {
  constexpr bool PEARSON = KIND == KIND_COMBINED, ABSL = KIND == KIND_CONTRASTIVE;
  __shared__ double mred[4][7];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = row_begin + blk * 4 + wv;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  double L = 0.0, sdt = 0.0, st = 0.0, stt = 0.0, dg = 0.0;   // the support's moment changes in fp64
  if (i < row_end) {   // wave-uniform
    const size_t ic = cmap ? (size_t)cmap[i] : (size_t)i;
    const float xi = coords[3 * ic], yi = coords[3 * ic + 1], zi = coords[3 * ic + 2];
    const int e1 = rowptr[i + 1];
    // four of the lane's entries per round, every index and coordinate load of the round issued before
    // its arithmetic (one wave per row: the col -> coordinate load chain was the pass's latency)
    constexpr int SU = 4;
    for (int e0 = rowptr[i] + lane; e0 < e1; e0 += 64 * SU) {
      int jj[SU];
      float tt[SU], cx[SU], cy[SU], cz[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int e = e0 + 64 * u;
        jj[u] = e < e1 ? col[e] : i;
        tt[u] = e < e1 ? val[e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const size_t jc = cmap ? (size_t)cmap[jj[u]] : (size_t)jj[u];
        // cpad: the coordinates as float4 rows (one 16-B load per lane instead of three 4-B loads)
        if (cpad) {
          const float4 c = cpad[jc];
          cx[u] = c.x; cy[u] = c.y; cz[u] = c.z;
        } else {
          cx[u] = coords[3 * jc]; cy[u] = coords[3 * jc + 1]; cz[u] = coords[3 * jc + 2];
        }
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        if (e0 + 64 * u >= e1) break;
        const int j = jj[u];
        const float t = tt[u];
        const float dx = xi - cx[u], dy = yi - cy[u], dz = zi - cz[u];
        const float d2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, 0x1.0p-100f)));
        const float inv = __builtin_amdgcn_rsqf(d2);
        const float d = d2 * inv;
        const float w = ABSL ? sgn_inv(d - t, inv) - sgn_inv(d - bg, inv) : (bg - t) * inv;
        gx = fmaf(w, dx, gx);
        gy = fmaf(w, dy, gy);
        gz = fmaf(w, dz, gz);
        if (j > i) {
          const double dd = d, td = t, bd = bg;
          const double r = dd - td, rb = dd - bd;
          L += ABSL ? fabs(r) - fabs(rb) : r * r - rb * rb;
          if (PEARSON) {
            sdt += dd * (td - bd);
            st += td - bd;
            stt += td * td - bd * bd;
          }
        }
      }
    }
    if (lane == 0 && !ABSL) {
      const float ti = diag[i];
      dg = (double)ti * (double)ti;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    gx += __shfl_xor(gx, o);
    gy += __shfl_xor(gy, o);
    gz += __shfl_xor(gz, o);
  }
  if (i < row_end && lane == 0) corr[i] = make_float4(gx, gy, gz, 0.f);
  // sum d and sum d^2 (1, 2) do not change; sdt, st, stt (3..5) only for the Pearson term
  double m[7] = {L, 0.0, 0.0, sdt, st, stt, dg};
  moment_wave_sums<7, PEARSON ? 0x79u : 0x41u>(m, mred, lane, wv);
  __syncthreads();
  moment_record<7>(mred, mom + (size_t)blk * 8);
}

// ---- tile prologue and epilogue, both chains ------------------------------------------------------

// The coordinate rows of row block I into sc[0] and of column block J into sc[1] (0 past N).  cmap:
// global row -> coords row (sharded step).  cpad: the diagonal tile of row block I writes its rows'
// float4 copy for the support pass that follows.
__device__ __forceinline__ void stage_coords(const float *__restrict__ coords, const int *__restrict__ cmap,
                                             float4 *__restrict__ cpad, int N, int I, int J, float (*sc)[BT][3]) {
  for (int k = threadIdx.x; k < 2 * BT; k += 256) {
    const int which = k / BT, li = k % BT;
    const int g = (which ? J : I) * BT + li;
    float x = 0.f, y = 0.f, z = 0.f;
    if (g < N) {
      const size_t gc = cmap ? (size_t)cmap[g] : (size_t)g;
      x = coords[3 * gc];
      y = coords[3 * gc + 1];
      z = coords[3 * gc + 2];
    }
    sc[which][li][0] = x;
    sc[which][li][1] = y;
    sc[which][li][2] = z;
    if (cpad && I == J && which == 0 && g < N) cpad[g] = make_float4(x, y, z, 0.f);
  }
}

// Column partials of P planes (a[plane]: the thread's 8 columns, summed in place): each value over the
// 4 ty of its wave (lanes l, l^16, l^32, l^48), then lanes < 16 write colred[plane][wave][column]; after
// a barrier col_sums adds the 4 waves in order.
template <int P>
__device__ __forceinline__ void col_partials(float *const (&a)[P], float (*colred)[4][BT], int tx, int lane, int wv) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
#pragma unroll
    for (int c = 0; c < P; ++c) a[c][q] = sum_rows4(a[c][q]);
  }
  if (lane < 16) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int lc = tx * 4 + (q & 3) + (q >> 2) * 64;
#pragma unroll
      for (int c = 0; c < P; ++c) colred[c][wv][lc] = a[c][q];
    }
  }
}

template <int P>
__device__ __forceinline__ void col_sums(const float (*colred)[4][BT], int lc, float (&s)[P]) {
#pragma unroll
  for (int c = 0; c < P; ++c) {
    s[c] = colred[c][0][lc];
#pragma unroll
    for (int w2 = 1; w2 < 4; ++w2) s[c] += colred[c][w2][lc];
  }
}

// Row lr of P rowpart planes: its 16 per-thread partials (four 16-B loads) added in tx order.
template <int P>
__device__ __forceinline__ void row_sums(const float *rowpart, int lr, float (&s)[P]) {
#pragma unroll
  for (int c = 0; c < P; ++c) {
    float v[16];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const float4 o = *reinterpret_cast<const float4 *>(&rowpart[c * kRowPlane + lr * kRowPad + 4 * q4]);
      v[4 * q4] = o.x; v[4 * q4 + 1] = o.y; v[4 * q4 + 2] = o.z; v[4 * q4 + 3] = o.w;
    }
    s[c] = v[0];
#pragma unroll
    for (int q = 1; q < 16; ++q) s[c] += v[q];   // tx order, as the 16 entries were always added
  }
}

// ---- the tile kernels -----------------------------------------------------------------------------

// The support pass riding in the background-form tile launch (SUP): blocks [ntiles, ntiles +
// blocks) of the grid run pairdist_support_kernel's work for support block (blockIdx.x - ntiles).
struct SupportArgs {
  const int32_t *rowptr = nullptr, *col = nullptr;
  const float *val = nullptr, *diag = nullptr;
  float4 *corr = nullptr;
  double *mom = nullptr;
  int row_begin = 0, row_end = 0;
  int64_t ntiles = 0;
};

// MODE_SYM: T = symmetric truth, tiles I <= J, pairs i < j, w = (d - t)/d (scale 4/N^2 later).
// MODE_FULL: T = upstream grad G of D, all tiles, pairs i != j, w = g/d.
// KIND: KIND_MSE: sum (d - t)^2; KIND_COMBINED: also the d / t moments of the Pearson term;
// KIND_CONTRASTIVE: sum |d - t| and w = sgn(d - t) / d.
// BG: the background form (T = bg at every pair; no T read, no diagonal term -- the support pass,
// pairdist_support_kernel, adds the entries that differ and the diagonal).
// The background form is latency-bound and is built for four workgroups per CU: <= 128 VGPRs (the
// launch bound makes the compiler hold to them) and <= 40 KB of LDS; tests/test_pairdist_resources_host.py
// checks both from the kernel metadata.
template <int MODE, bool VEC, int KIND, bool BG = false, bool SUP = false>
__global__ __launch_bounds__(256, BG ? 4 : 1) void pairdist_tile_kernel(const float *__restrict__ coords,
                                                            const float *__restrict__ T, int N,
                                                            int64_t ldt, int64_t row0, int64_t col0,
                                                            int nb, int64_t t0,
                                                            float4 *__restrict__ part,
                                                            double *__restrict__ mom, float bg,
                                                            const int *__restrict__ cmap = nullptr,
                                                            const SupportArgs sup = SupportArgs{},
                                                            float4 *__restrict__ cpad = nullptr) {
  static_assert(!BG || (MODE == MODE_SYM && !VEC), "the background form is the training loss without a T image");
  static_assert(!SUP || BG, "the support pass rides only in the background form's launch");
  if (SUP && (int64_t)blockIdx.x >= sup.ntiles) {   // block-uniform
    support_block<KIND>(coords, bg, sup.row_begin, sup.row_end, sup.rowptr, sup.col, sup.val, sup.diag, sup.corr,
                           sup.mom, cmap, (int)(blockIdx.x - sup.ntiles));
    return;
  }
  // one dynamic LDS array: [T tile 128x128 fp32 (VEC only)] -- 64 KiB, 16-B aligned
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ float sc[2][BT][3];
  __shared__ float colred[3][4][BT];   // planar x / y / z: [wave][column]
  __shared__ double mred[4][7];
  constexpr bool RL = BG;
  __shared__ __attribute__((aligned(16))) float rowpart_s[RL ? 3 * kRowPlane : 1];
  float *rowpart = RL ? rowpart_s : nullptr;
  const int64_t t = t0 + blockIdx.x;
  int I, J;
  if (MODE == MODE_SYM) {
    tri_decode(t, nb, I, J);
  } else {
    I = (int)(t / nb);
    J = (int)(t % nb);
  }
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wv = tid >> 6;
  stage_coords(coords, cmap, cpad, N, I, J, sc);
  if (VEC) {
    // LDS-DMA of the T tile (global_load_lds_dwordx4: each wave instruction moves 1 KiB = two 512-B
    // tile rows, wave-uniform LDS base + lane*16), each wave only the 32 rows its threads read:
    // rows 16w .. 16w+15 (k = 0..3 of tile_rows) first, then 64+16w .. 64+16w+15 (k = 4..7), so the
    // first half is computed while the second is in flight.  Rows past N are clamped to a valid row
    // (their values are masked); columns past N lie inside the padded leading dimension.  T may be
    // a band of the truth (rows from row0, columns from col0: a rank's share, hicgat.dist).
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r0 = (q < 8 ? 0 : 64) + wv * 16 + (q & 7) * 2;
      const int gi = min(I * BT + r0 + (lane >> 5), N - 1);
      const float *src = T + (size_t)(gi - row0) * ldt + (size_t)((int64_t)J * BT - col0) + (lane & 31) * 4;
      __builtin_amdgcn_global_load_lds(src, &tile[r0 * BT], 16, 0, 0);
    }
  }
  // sc[] (written above with ds_write) to all waves: LDS drain + raw barrier -- __syncthreads()
  // would also drain vmcnt and so wait for the whole tile
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  float cx[8], cy[8], cz[8];
  const int gj0 = J * BT + tx * 4;
  TileAcc A;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int lc = tx * 4 + (q & 3) + (q >> 2) * 64;
    cx[q] = sc[1][lc][0];
    cy[q] = sc[1][lc][1];
    cz[q] = sc[1][lc][2];
    A.ax[q] = A.ay[q] = A.az[q] = 0.f;
  }
  float4 *prow = part + (size_t)t * 2 * BT;
  const bool interior = I != J && (I + 1) * BT <= N && (J + 1) * BT <= N;   // block-uniform
  if (VEC) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");    // this wave's first 16 rows landed
  constexpr bool PK = (VEC || BG) && MODE == MODE_SYM;   // packed interior path (tile_rows_pk)
  if constexpr (BG) {
    // no T image to wait for between the halves: one branch around both, so the interior and the
    // masked form never share a live range (the two half-calls stay: each half's moments are
    // summed on their own and then added, the order the records have always had)
    if (interior) {
      tile_rows_pk<KIND, 0, 4, BG, RL>(tile, bg, sc, tx, ty, cx, cy, cz, prow, A, rowpart);
      tile_rows_pk<KIND, 4, 8, BG, RL>(tile, bg, sc, tx, ty, cx, cy, cz, prow, A, rowpart);
    } else {
      tile_rows<MODE, VEC, KIND, true, 0, 4, BG, RL>(T, ldt, row0, col0, N, I, J, bg, tile, sc, tx, ty, cx, cy, cz, gj0, prow, A, rowpart);
      tile_rows<MODE, VEC, KIND, true, 4, 8, BG, RL>(T, ldt, row0, col0, N, I, J, bg, tile, sc, tx, ty, cx, cy, cz, gj0, prow, A, rowpart);
    }
  } else {
    if (interior) {
      if constexpr (PK) tile_rows_pk<KIND, 0, 4, BG, RL>(tile, bg, sc, tx, ty, cx, cy, cz, prow, A, rowpart);
      else tile_rows<MODE, VEC, KIND, false, 0, 4>(T, ldt, row0, col0, N, I, J, bg, tile, sc, tx, ty, cx, cy, cz, gj0, prow, A, rowpart);
    } else {
      tile_rows<MODE, VEC, KIND, true, 0, 4, BG, RL>(T, ldt, row0, col0, N, I, J, bg, tile, sc, tx, ty, cx, cy, cz, gj0, prow, A, rowpart);
    }
    if (VEC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // and the second 16
    if (interior) {
      if constexpr (PK) tile_rows_pk<KIND, 4, 8, BG, RL>(tile, bg, sc, tx, ty, cx, cy, cz, prow, A, rowpart);
      else tile_rows<MODE, VEC, KIND, false, 4, 8>(T, ldt, row0, col0, N, I, J, bg, tile, sc, tx, ty, cx, cy, cz, gj0, prow, A, rowpart);
    } else {
      tile_rows<MODE, VEC, KIND, true, 4, 8, BG, RL>(T, ldt, row0, col0, N, I, J, bg, tile, sc, tx, ty, cx, cy, cz, gj0, prow, A, rowpart);
    }
  }

  float *const planes[3] = {A.ax, A.ay, A.az};
  col_partials<3>(planes, colred, tx, lane, wv);
  if (MODE == MODE_SYM) {
    // the Pearson moments (1..5) only for the combined loss; the others stay 0 in every lane
    double m[7] = {A.L, A.sd, A.sdd, A.sdt, A.st, A.stt, A.dg};
    moment_wave_sums<7, KIND == KIND_COMBINED ? 0x7Fu : 0x41u>(m, mred, lane, wv);
  }
  __syncthreads();
  float s[3];
  if (tid < BT) {
    col_sums<3>(colred, tid, s);
    prow[BT + tid] = make_float4(s[0], s[1], s[2], 0.f);
  } else if (RL) {   // the other forms took their row partials from sum16 inside the pair loop
    row_sums<3>(rowpart, tid - BT, s);
    prow[tid - BT] = make_float4(s[0], s[1], s[2], 0.f);
  }
  if (MODE == MODE_SYM) moment_record<7>(mred, mom + (size_t)t * 8);
}

template <int KIND>
__global__ __launch_bounds__(256) void pairdist_support_kernel(const float *__restrict__ coords, int N, float bg,
                                                               int row_begin, int row_end,
                                                               const int32_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ col,
                                                               const float *__restrict__ val,
                                                               const float *__restrict__ diag,
                                                               float4 *__restrict__ corr, double *__restrict__ mom,
                                                               const int *__restrict__ cmap,
                                                               const float4 *__restrict__ cpad = nullptr) {
  support_block<KIND>(coords, bg, row_begin, row_end, rowptr, col, val, diag, corr, mom, cmap, blockIdx.x, cpad);
}

// D[i, j] = ||c_i - c_j||: one thread per element.
__global__ __launch_bounds__(256) void pairdist_fwd_kernel(const float *__restrict__ coords, int N,
                                                           float *__restrict__ D, int64_t ldd) {
  __shared__ float ci[3];
  const int i = blockIdx.y;
  if (threadIdx.x < 3) ci[threadIdx.x] = coords[3 * (size_t)i + threadIdx.x];
  __syncthreads();
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const float dx = ci[0] - coords[3 * (size_t)j], dy = ci[1] - coords[3 * (size_t)j + 1],
              dz = ci[2] - coords[3 * (size_t)j + 2];
  D[(size_t)i * ldd + j] = i == j ? 0.f : sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
}

// One 256-thread block per upper-triangle 128x128 tile, whole matrix only.  Writes, per tile, four
// [128] float4 slabs (R row partials, R column partials, W row partials, W column partials) and one
// moment record of 8 doubles: sum (d-t)^2, sum d, sum d^2, sum dt, sum t, sum t^2, sum T_ii^2,
// sum T_ii.  Two workgroups per CU (256 VGPRs, ~77 KB of LDS).
template <bool BG>
__global__ __launch_bounds__(256, 2) void pairdist_mloss_tile_kernel(const float *__restrict__ coords,
                                                                     const float *__restrict__ T, int N, int64_t ldt,
                                                                     int vec, int nb, float4 *__restrict__ part,
                                                                     double *__restrict__ mom, float bg,
                                                                     float4 *__restrict__ cpad) {
  __shared__ float sc[2][BT][3];
  __shared__ float colred[kMPlanes][4][BT];
  __shared__ double mred[4][8];
  __shared__ __attribute__((aligned(16))) float rowpart[kMPlanes * kRowPlane];
  const int64_t t = blockIdx.x;
  int I, J;
  tri_decode(t, nb, I, J);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wv = tid >> 6;
  stage_coords(coords, nullptr, cpad, N, I, J, sc);
  __syncthreads();

  f2 cx2[4], cy2[4], cz2[4];
  const int gj0 = J * BT + tx * 4;
  MTileAcc A;
  const f2 z2 = f2{0.f, 0.f};
  A.L = A.sd = A.sdd = A.sdt = A.st = A.stt = z2;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int lc0 = tx * 4 + ((2 * h) & 3) + ((2 * h) >> 2) * 64;
    cx2[h] = f2{sc[1][lc0][0], sc[1][lc0 + 1][0]};
    cy2[h] = f2{sc[1][lc0][1], sc[1][lc0 + 1][1]};
    cz2[h] = f2{sc[1][lc0][2], sc[1][lc0 + 1][2]};
    A.ax[h] = A.ay[h] = A.az[h] = A.bx[h] = A.by[h] = A.bz[h] = z2;
  }
  const bool interior = I != J && (I + 1) * BT <= N && (J + 1) * BT <= N;   // block-uniform
  if (interior) {
    mloss_rows<false, BG>(T, ldt, vec != 0, N, I, J, bg, sc, tx, ty, cx2, cy2, cz2, gj0, A, rowpart);
    if constexpr (BG) {   // 64 pairs per thread, all at bg
      const f2 sd = A.sd;
      A.sdt = f2{bg * sd.x, bg * sd.y};
      A.st = f2{32.f * bg, 32.f * bg};
      A.stt = f2{32.f * bg * bg, 32.f * bg * bg};
    }
  } else {
    mloss_rows<true, BG>(T, ldt, vec != 0, N, I, J, bg, sc, tx, ty, cx2, cy2, cz2, gj0, A, rowpart);
  }

  float a[kMPlanes][8];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    a[0][2 * h] = A.ax[h].x; a[0][2 * h + 1] = A.ax[h].y;
    a[1][2 * h] = A.ay[h].x; a[1][2 * h + 1] = A.ay[h].y;
    a[2][2 * h] = A.az[h].x; a[2][2 * h + 1] = A.az[h].y;
    a[3][2 * h] = A.bx[h].x; a[3][2 * h + 1] = A.bx[h].y;
    a[4][2 * h] = A.by[h].x; a[4][2 * h + 1] = A.by[h].y;
    a[5][2 * h] = A.bz[h].x; a[5][2 * h + 1] = A.bz[h].y;
  }
  float *const planes[kMPlanes] = {a[0], a[1], a[2], a[3], a[4], a[5]};
  col_partials<kMPlanes>(planes, colred, tx, lane, wv);
  double m[8] = {(double)A.L.x + (double)A.L.y,     (double)A.sd.x + (double)A.sd.y,
                 (double)A.sdd.x + (double)A.sdd.y, (double)A.sdt.x + (double)A.sdt.y,
                 (double)A.st.x + (double)A.st.y,   (double)A.stt.x + (double)A.stt.y,
                 A.dg,                              A.sg};
  moment_wave_sums<8>(m, mred, lane, wv);
  __syncthreads();
  float4 *prow = part + (size_t)t * 4 * BT;   // slabs: R rows, R columns, W rows, W columns
  float s[kMPlanes];
  if (tid < BT) {
    col_sums<kMPlanes>(colred, tid, s);
    prow[BT + tid] = make_float4(s[0], s[1], s[2], 0.f);
    prow[3 * BT + tid] = make_float4(s[3], s[4], s[5], 0.f);
  } else {
    row_sums<kMPlanes>(rowpart, tid - BT, s);
    prow[tid - BT] = make_float4(s[0], s[1], s[2], 0.f);
    prow[2 * BT + tid - BT] = make_float4(s[3], s[4], s[5], 0.f);
  }
  moment_record<8>(mred, mom + (size_t)t * 8);
}

// ---- second stage: per-row slab sums and moment partials ------------------------------------------

constexpr int kRedGroups = 16;   // J-groups per row in the reduce kernels (1024-thread blocks)

// Tile moments in two fixed-order stages (deterministic): kMomBlocks extra blocks of the reduce kernel
// each sum a contiguous run of records (moments_partial_block) into mpart[b][0..M); the finalize adds
// the kMomBlocks partials in block order.  A rank's share whose partial moments are all-reduced before
// the finalize (the sharded step) with at most kOneBlockMoments records: ONE such block writes
// stats[0..6] itself (no moments_finalize launch).
constexpr int kMomBlocks = 64;
constexpr int64_t kOneBlockMoments = 4096;

// Row lr of row block R: group grp's share (J = grp, grp + kRedGroups, ...) of the S sums over the
// tiles touching the row -- sum s adds slab 2s (row partials) of tile (R, J) and slab 2s + 1 (column
// partials) of tile (J, R), of 2S [128] float4 slabs per tile; only tiles in [t0, t1).  MODE_SYM:
// upper-triangle tiles, so the row slab for J >= R and the column slab for J <= R.
template <int S>
__device__ __forceinline__ void gather_row(const float4 *__restrict__ part, int nb, int mode, int64_t t0, int64_t t1,
                                           int R, int lr, int grp, float4 (&sum)[S]) {
  const size_t st = (size_t)(2 * S) * BT;
#pragma unroll 2
  for (int J = grp; J < nb; J += kRedGroups) {
    int64_t trow, tcol;
    if (mode == MODE_SYM) {
      trow = J >= R ? tri_start(R, nb) + (J - R) : -1;
      tcol = J <= R ? tri_start(J, nb) + (R - J) : -1;
    } else {
      trow = (int64_t)R * nb + J;
      tcol = (int64_t)J * nb + R;
    }
    const bool has_row = trow >= t0 && trow < t1, has_col = tcol >= t0 && tcol < t1;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (has_row) a = part[(size_t)trow * st + (2 * s) * BT + lr];
      if (has_col) b = part[(size_t)tcol * st + (2 * s + 1) * BT + lr];
      add3(sum[s], a);
      add3(sum[s], b);
    }
  }
}

// the kRedGroups group sums red[group][64] of one row, added in group order
__device__ __forceinline__ float4 group_sum(const float4 *red, int lr64) {
  float4 s = red[lr64];
#pragma unroll
  for (int g = 1; g < kRedGroups; ++g) add3(s, red[g * 64 + lr64]);
  return s;
}

// Block blk of nblk sums its run of the moment records [t0, t1) into part[blk][0..M): 256 threads, each
// a strided subset with its loads in flight, then a fixed tree over buf [M][256].  M = 8: component 7
// only over the records below t7 (the tiles: the support pass's records have no such entry).
template <int M>
__device__ __forceinline__ void moments_partial_block(const double *__restrict__ mom, int64_t t0, int64_t t1,
                                                      int64_t t7, int blk, int nblk, double *__restrict__ part,
                                                      double *buf) {
  const int tid = threadIdx.x;
  const int64_t per = (t1 - t0 + nblk - 1) / nblk;
  const int64_t b0 = t0 + (int64_t)blk * per, b1 = min(t1, b0 + per);
  if (tid < 256) {
    double s[M] = {};
    for (int64_t t = b0 + tid; t < b1; t += 256) {
#pragma unroll
      for (int c = 0; c < 7; ++c) s[c] += mom[(size_t)t * 8 + c];
      if (M == 8 && t < t7) s[M - 1] += mom[(size_t)t * 8 + 7];
    }
#pragma unroll
    for (int c = 0; c < M; ++c) buf[c * 256 + tid] = s[c];
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int c = 0; c < M; ++c) buf[c * 256 + tid] += buf[c * 256 + tid + o];
    }
    __syncthreads();
  }
  if (tid < M) part[blk * 8 + tid] = buf[tid * 256];
}

// dcoords[i] = scale * (sum of the row partials of tiles (R, *) + column partials of (*, R)), the slab
// of a tile being [row partials | column partials].  Block = 64 rows x kRedGroups groups; the group
// sums are combined in group order (fixed order: bitwise reproducible), then the support pass's
// per-row term corr (background form).
// mom != NULL: the blocks from row_blocks on (gridDim.x - row_blocks of them) sum runs of the moment
// records [m0, m1) (tiles, then the support pass's blocks) into mpart instead (moments_partial_block).
__global__ __launch_bounds__(1024) void pairdist_reduce_kernel(const float4 *__restrict__ part, int N, int nb,
                                                               int mode, int64_t t0, int64_t t1, float scale,
                                                               float *__restrict__ dcoords,
                                                               const double *__restrict__ mom, int64_t m0, int64_t m1,
                                                               int row_blocks, double *__restrict__ mpart,
                                                               const float4 *__restrict__ corr, int corr_r0,
                                                               int corr_r1, double *__restrict__ dc64) {
  if (mom && (int)blockIdx.x >= row_blocks) {
    __shared__ double mbuf[7 * 256];
    moments_partial_block<7>(mom, m0, m1, 0, (int)blockIdx.x - row_blocks, (int)gridDim.x - row_blocks, mpart, mbuf);
    return;
  }
  __shared__ float4 red[kRedGroups * 64];
  const int lr64 = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int gi = blockIdx.x * 64 + lr64;
  float4 sum[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
  if (gi < N) gather_row<1>(part, nb, mode, t0, t1, gi / BT, gi % BT, grp, sum);
  red[grp * 64 + lr64] = sum[0];
  __syncthreads();
  if (grp == 0 && gi < N) {
    float4 s0 = group_sum(red, lr64);
    if (corr && gi >= corr_r0 && gi < corr_r1) add3(s0, corr[gi]);
    const float gx = s0.x * scale, gy = s0.y * scale, gz = s0.z * scale;
    if (dc64) {   // the fp32 values, widened: straight into a caller's fp64 all-reduce buffer
      dc64[3 * (size_t)gi] = gx;
      dc64[3 * (size_t)gi + 1] = gy;
      dc64[3 * (size_t)gi + 2] = gz;
    } else {
      dcoords[3 * (size_t)gi] = gx;
      dcoords[3 * (size_t)gi + 1] = gy;
      dcoords[3 * (size_t)gi + 2] = gz;
    }
  }
}

// The moment-dependent chain's second stage, one launch of 1024-thread blocks over the whole range:
//   blocks [0, row_blocks): R_i and W_i of 64 rows each (gather_row, the group sums in group order,
//     then corr[i], the support pass's change of R_i, background form) into rw[i] (R) and rw[N + i] (W);
//   blocks [row_blocks, row_blocks + kMomBlocks): runs of the moment records [0, m_all), component 7
//     over the m_tiles tile records only;
//   the last block: sum_j c_j (x, y, z) and sum_i diag[i] (background form; else 0) in fp64 -> csum[4].
// Every sum has a fixed order.
__global__ __launch_bounds__(1024) void pairdist_mloss_reduce_kernel(const float4 *__restrict__ part, int N, int nb,
                                                                     float4 *__restrict__ rw,
                                                                     const double *__restrict__ mom, int64_t m_tiles,
                                                                     int64_t m_all, int row_blocks,
                                                                     double *__restrict__ mpart,
                                                                     const float4 *__restrict__ corr,
                                                                     const float *__restrict__ coords,
                                                                     const float *__restrict__ diag,
                                                                     double *__restrict__ csum) {
  __shared__ __attribute__((aligned(16))) double shbuf[4 * 1024];   // 32 KB, one use per block kind
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  if (blk >= row_blocks + kMomBlocks) {   // coordinate and diagonal sums
    double s[4] = {0, 0, 0, 0};
    for (int j = tid; j < N; j += 1024) {
      s[0] += (double)coords[3 * (size_t)j];
      s[1] += (double)coords[3 * (size_t)j + 1];
      s[2] += (double)coords[3 * (size_t)j + 2];
      if (diag) s[3] += (double)diag[j];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) shbuf[c * 1024 + tid] = s[c];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if (tid < o) {
#pragma unroll
        for (int c = 0; c < 4; ++c) shbuf[c * 1024 + tid] += shbuf[c * 1024 + tid + o];
      }
      __syncthreads();
    }
    if (tid < 4) csum[tid] = shbuf[tid * 1024];
    return;
  }
  if (blk >= row_blocks) {
    moments_partial_block<8>(mom, 0, m_all, m_tiles, blk - row_blocks, kMomBlocks, mpart, shbuf);
    return;
  }
  float4 *red = reinterpret_cast<float4 *>(shbuf);   // [2][kRedGroups][64]
  const int lr64 = tid & 63, grp = tid >> 6;
  const int gi = blk * 64 + lr64;
  float4 sum[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};   // R, W
  if (gi < N) gather_row<2>(part, nb, (int)MODE_SYM, 0, INT64_MAX, gi / BT, gi % BT, grp, sum);
  red[grp * 64 + lr64] = sum[0];
  red[(kRedGroups + grp) * 64 + lr64] = sum[1];
  __syncthreads();
  if (grp == 0 && gi < N) {
    float4 r0 = group_sum(red, lr64);
    if (corr) add3(r0, corr[gi]);
    rw[gi] = r0;
    rw[(size_t)N + gi] = group_sum(red + kRedGroups * 64, lr64);
  }
}

// ---- finalize -------------------------------------------------------------------------------------

// threads < M: the kMomBlocks partials of component threadIdx.x, added in block order
template <int M>
__device__ __forceinline__ void sum_moment_partials(const double *__restrict__ mpart, double *dst) {
  if (threadIdx.x < M) {
    double s = 0.0;
    for (int b = 0; b < kMomBlocks; ++b) s += mpart[b * 8 + threadIdx.x];
    dst[threadIdx.x] = s;
  }
}

// What both chains form from the moments s[0..6] = L, sd, sdd, sdt, st, stt, dg: the MSE over all N^2
// entries, the pair count M, and the covariance and variances of d and t over the pairs (times M).
// Pearson r = cov / sqrt(vd vt) is left to the callers: the two chains differ in when it is defined.
struct MomentStats {
  double mse, M, cov, vd, vt;
};

__device__ __forceinline__ MomentStats moment_stats(int N, const double *s) {
  const double n2 = (double)N * (double)N;
  MomentStats m;
  m.mse = (2.0 * s[0] + s[6]) / n2;
  m.M = 0.5 * (double)N * (double)(N - 1);
  const double sd = s[1], sdd = s[2], sdt = s[3], st = s[4], stt = s[5];
  m.cov = sdt - sd * st / m.M;
  m.vd = sdd - sd * sd / m.M;
  m.vt = stt - st * st / m.M;
  return m;
}

// stats[7..10] and loss from the (all-reduced) moments stats[0..6]: mse, pearson r, alpha, total;
// contrastive: stats[7] = mean_{i<j} |T - D| (fp64, as the reference's float64 truth makes it),
// stats[8] = NaN, stats[9] = 0.1, stats[10] = total = 0.1 * stats[7].
__device__ void finalize_stats(int N, int loss_kind, double *__restrict__ stats, float *__restrict__ loss) {
  if (loss_kind == KIND_CONTRASTIVE) {
    const double M = 0.5 * (double)N * (double)(N - 1);
    const double mae = M > 0.0 ? stats[0] / M : 0.0;
    const double total = 0.1 * mae;
    stats[7] = mae;
    stats[8] = NAN;
    stats[9] = 0.1;
    stats[10] = total;
    stats[11] = 0.0;
    if (loss) loss[0] = (float)total;
    return;
  }
  const MomentStats ms = moment_stats(N, stats);
  const double mse = ms.mse;
  // r is reported, never differentiated here (the reference's Pearson term is detached): any positive
  // pair of variances gives a value.  The moment-dependent chain, which divides its gradient by them,
  // asks for more (kVarFloor, pairdist_mloss_finalize_kernel).
  const double r = (ms.vd > 0.0 && ms.vt > 0.0) ? ms.cov / sqrt(ms.vd * ms.vt) : NAN;
  // HiC_GAT_generalize_directly.py:223-225: alpha from mse_loss.item() (the fp32 value), then
  // total_loss = mse_loss + alpha*(1-r) evaluated as an fp32 tensor + scalar add.
  const float msef = (float)mse;
  const double alpha = fmin(1.0, 0.1 + 1.0 / ((double)msef + 1e-6));
  const float totalf = msef + (float)(alpha * (1.0 - r));
  stats[7] = mse;
  stats[8] = r;
  stats[9] = alpha;
  stats[10] = (double)totalf;
  stats[11] = 0.0;
  if (loss) loss[0] = loss_kind == 1 ? totalf : msef;
}

__global__ __launch_bounds__(64) void finalize_kernel(int N, int loss_kind, double *__restrict__ stats,
                                                      float *__restrict__ loss) {
  if (threadIdx.x == 0) finalize_stats(N, loss_kind, stats, loss);
}

__global__ __launch_bounds__(64) void moments_finalize_kernel(const double *__restrict__ part, int N, int loss_kind,
                                                              double *__restrict__ stats, float *__restrict__ loss) {
  sum_moment_partials<7>(part, stats);
  __syncthreads();
  if (threadIdx.x == 0) finalize_stats(N, loss_kind, stats, loss);
}

// finalize + a rank's rows of the all-reduced fp64 dcoords narrowed to fp32 (one launch after the
// multi-GPU loss all-reduce instead of two); with cbuf, also the coordinates in global row order,
// cglob[i] = cbuf[gidx[i]] (the padded all-gather layout reordered: step()'s return value, no launch
// of its own)
__global__ __launch_bounds__(256) void finalize_rows_kernel(int N, int loss_kind, double *__restrict__ stats,
                                                            float *__restrict__ loss, const double *__restrict__ dc64,
                                                            int64_t n3, float *__restrict__ dcoords,
                                                            const float *__restrict__ cbuf,
                                                            const int32_t *__restrict__ gidx, float *__restrict__ cglob) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) finalize_stats(N, loss_kind, stats, loss);
  if (t < n3) dcoords[t] = (float)dc64[t];
  if (cbuf && t < 3 * (int64_t)N) {
    const int64_t i = t / 3;
    cglob[t] = cbuf[3 * (int64_t)gidx[i] + (t - 3 * i)];
  }
}

// Finalize + combine of the moment-dependent chain, one launch.  Every block adds the kMomBlocks moment
// partials in block order (the same bits in every block), forms mse, r, the loss value and the
// coefficients A, B, C of g_ij = A d_ij + B t_ij + C in fp64, and then gives its 256 rows
//   dcoords[i] = float(-B R_i + (A + B) (N c_i - sum_j c_j) + C W_i).
// Block 0 writes stats[0..11] and loss.  stats: 0..6 the moments as hicgat_pairdist_mse_fused,
// 7 mse, 8 pearson r (NaN when a variance is <= 0), 9 alpha (PEARSON) / 0 (RMSE) / mean of D - T over
// all entries (SI_MSE), 10 the loss value, 11 sum_i T_ii.
__global__ __launch_bounds__(256) void pairdist_mloss_finalize_kernel(const double *__restrict__ mpart,
                                                                      const double *__restrict__ csum,
                                                                      const float4 *__restrict__ rw,
                                                                      const float *__restrict__ coords, int N,
                                                                      int kind, double alpha,
                                                                      double *__restrict__ stats,
                                                                      float *__restrict__ loss,
                                                                      float *__restrict__ dcoords) {
  __shared__ double sm[8];
  __shared__ double coef[3];
  const int tid = threadIdx.x;
  sum_moment_partials<8>(mpart, sm);
  __syncthreads();
  if (tid == 0) {
    const MomentStats ms = moment_stats(N, sm);
    const double n2 = (double)N * (double)N, M = ms.M;
    const double sd = sm[1], sdd = sm[2], st = sm[4], stt = sm[5];
    const double sdiag = sm[7] + csum[3];
    const double mse = ms.mse, vd = ms.vd, vt = ms.vt;
    // unlike finalize_stats, r feeds the gradient here (1 / vd, 1 / sqrt(vd vt)): the tile sums are fp32
    // per thread, so a variance below 2^-20 of the mean square is their rounding (N = 2: fl(d^2) - d^2),
    // not a spread, and counts as <= 0
    double r = NAN;
    if (M > 0.0 && vd > kVarFloor * sdd && vt > kVarFloor * stt) r = ms.cov / sqrt(vd * vt);
    const double g4 = 4.0 / n2;
    const double rmse = sqrt(mse + 1e-12);
    const double ebar = (2.0 * (sd - st) - sdiag) / n2;   // the all-entries mean of D - T
    // g_ij = A d_ij + B t_ij + C: the MSE part (halved by the root for RMSE), then the kind's own terms
    const double base = kind == MLOSS_RMSE ? g4 / (2.0 * rmse) : g4;
    double ea = 0.0, eb = 0.0, c = 0.0;
    const bool pearson = kind == MLOSS_PEARSON && r == r;   // a variance <= 0: no gradient through the term
    if (pearson) {
      const double isq = 1.0 / sqrt(vd * vt);
      ea = alpha * r / vd;
      eb = alpha * isq;
      c = alpha * ((st / M) * isq - r * (sd / M) / vd);
    }
    if (kind == MLOSS_SI_MSE) c = -g4 * ebar;
    const double a = base + ea, b = -(base + eb);
    double total, s9;
    if (kind == MLOSS_PEARSON) {
      total = mse + alpha * (pearson ? 1.0 - r : 1.0);   // r taken as 0 when it is undefined
      s9 = alpha;
    } else if (kind == MLOSS_RMSE) {
      total = rmse;
      s9 = 0.0;
    } else {
      total = mse - ebar * ebar;
      s9 = ebar;
    }
    coef[0] = a;
    coef[1] = b;
    coef[2] = c;
    if (blockIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 7; ++k) stats[k] = sm[k];
      stats[7] = mse;
      stats[8] = r;
      stats[9] = s9;
      stats[10] = total;
      stats[11] = sdiag;
      if (loss) loss[0] = (float)total;
    }
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + tid;
  if (dcoords && i < N) {
    const double a = coef[0], b = coef[1], c = coef[2];
    const float4 R = rw[i], W = rw[(size_t)N + i];
    const double nn = (double)N;
    const double ux = nn * (double)coords[3 * (size_t)i] - csum[0];
    const double uy = nn * (double)coords[3 * (size_t)i + 1] - csum[1];
    const double uz = nn * (double)coords[3 * (size_t)i + 2] - csum[2];
    dcoords[3 * (size_t)i] = (float)(-b * (double)R.x + (a + b) * ux + c * (double)W.x);
    dcoords[3 * (size_t)i + 1] = (float)(-b * (double)R.y + (a + b) * uy + c * (double)W.y);
    dcoords[3 * (size_t)i + 2] = (float)(-b * (double)R.z + (a + b) * uz + c * (double)W.z);
  }
}

}  // namespace hicgat

using namespace hicgat;

// ---- host: workspace layout -----------------------------------------------------------------------

constexpr size_t kTileLds = (size_t)BT * BT * sizeof(float);  // LDS image of one T tile

// mode: HICGAT_PD_TRI (1) = the upper-triangle tiling of the fused loss, HICGAT_PD_SQUARE (0) =
// the square tiling of the backward -- one convention for both queries (include/hicgat.h).
extern "C" int64_t hicgat_pairdist_num_tiles(int N, int mode) {
  if (N <= 0) return 0;
  const int64_t nb = pd_nb(N);
  return mode == HICGAT_PD_TRI ? nb * (nb + 1) / 2 : nb * nb;
}

static int64_t pd_support_blocks(int N) { return (N + 3) / 4; }   // support_block: 4 rows (waves) per block

// Byte offsets of a chain's workspace, in this order: [tiles][slabs][128] float4 partial slabs | one
// 8-double moment record per tile and (support) per support block: tiles [tile_begin, tile_end) at
// their tile index, the support blocks right after tile_end, so a share's records are one contiguous
// run that never passes tiles + pd_support_blocks(N) | kMomBlocks moment partials | mloss: csum[4]
// doubles, rw [2][N] float4 | support: corr [N] float4, the float4 coordinates cpad [N] | 256 spare.
// The size queries return total; the entry points carve with the same offsets.
struct PdLayout {
  size_t part, mom, mpart, csum, rw, corr, cpad, total;
};

static PdLayout pd_layout(int N, int mode, int slabs, bool support, bool mloss) {
  const size_t tiles = (size_t)hicgat_pairdist_num_tiles(N, mode), n = N > 0 ? (size_t)N : 0;
  const size_t f4 = sizeof(float4), rec = 8 * sizeof(double);
  size_t end = 0;
  const auto take = [&end](size_t bytes) {
    const size_t at = end;
    end += bytes;
    return at;
  };
  PdLayout L;
  L.part = take(tiles * slabs * BT * f4);
  L.mom = take((tiles + (support ? (size_t)pd_support_blocks((int)n) : 0)) * rec);
  L.mpart = take(kMomBlocks * rec);
  L.csum = take(mloss ? 4 * sizeof(double) : 0);
  L.rw = take(mloss ? 2 * n * f4 : 0);
  L.corr = take(support ? n * f4 : 0);
  L.cpad = take(support ? n * f4 : 0);
  L.total = end + 256;
  return L;
}

static PdLayout fused_layout(int N, int mode, bool support) { return pd_layout(N, mode, 2, support, false); }
static PdLayout mloss_layout(int N, bool support) { return pd_layout(N, HICGAT_PD_TRI, 4, support, true); }

template <class T>
static T *ws_at(void *ws, size_t offset) {
  return reinterpret_cast<T *>(static_cast<char *>(ws) + offset);
}

extern "C" size_t hicgat_pairdist_workspace_bytes(int N, int mode) { return fused_layout(N, mode, false).total; }
extern "C" size_t hicgat_pairdist_support_workspace_bytes(int N) {
  return N <= 0 ? 256 : fused_layout(N, HICGAT_PD_TRI, true).total;
}
extern "C" size_t hicgat_pairdist_moment_loss_workspace_bytes(int N) {
  return N <= 0 ? 256 : mloss_layout(N, false).total;
}
extern "C" size_t hicgat_pairdist_moment_loss_support_workspace_bytes(int N) {
  return N <= 0 ? 256 : mloss_layout(N, true).total;
}

// ---- host: entry points ---------------------------------------------------------------------------

// the per-pair gradient factor the reduction applies: MSE over N^2 entries of the symmetric D
// (each pair twice, d(d - t)^2 = 2 (d - t)): 4 / N^2; contrastive: 0.1 / M, M = N (N - 1) / 2 pairs --
// float32(0.1 / M), the value the reference's autograd hands to cdist's backward
static float loss_scale(int N, int loss_kind) {
  if (loss_kind == KIND_CONTRASTIVE) return N > 1 ? (float)(0.1 / (0.5 * (double)N * (double)(N - 1))) : 0.f;
  return (float)(4.0 / ((double)N * (double)N));
}

// Host twin of tri_decode (exact integer search): tile-row of upper-triangle tile t.
static int tri_row_host(int64_t t, int nb) {
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (tri_start(mid, nb) <= t) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// A [begin, end) argument (tiles, support rows): end < 0 or past limit means limit, begin < 0 means 0;
// false when the range is inverted.
static bool clamp_range(int64_t &begin, int64_t &end, int64_t limit) {
  if (end < 0 || end > limit) end = limit;
  if (begin < 0) begin = 0;
  return begin <= end;
}

// T (or G) can be read as 16-byte rows of whole tiles: the LDS image of pairdist_tile_kernel<VEC>, the
// float4 loads of mloss_rows.  col0: the column of the truth that T's first column holds.
static bool t_is_vec(const float *T, int64_t ld, int64_t col0, int nb) {
  return (ld % 4 == 0) && (col0 % 4 == 0) && ((reinterpret_cast<uintptr_t>(T) & 15) == 0) &&
         ld >= (int64_t)nb * BT - col0;
}

// f(std::integral_constant<int, KIND>) for the runtime loss kind
template <class F>
static void with_kind(int loss_kind, F &&f) {
  if (loss_kind == KIND_COMBINED) f(std::integral_constant<int, KIND_COMBINED>{});
  else if (loss_kind == KIND_CONTRASTIVE) f(std::integral_constant<int, KIND_CONTRASTIVE>{});
  else f(std::integral_constant<int, KIND_MSE>{});
}

static bool loss_kind_ok(int k) { return k >= KIND_MSE && k <= KIND_CONTRASTIVE; }

extern "C" int hicgat_pairdist_fwd(const float *coords, int N, float *D, int64_t ldd,
                                   hicgat_stream_t stream) {
  if (N < 0 || ldd < N) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!coords || !D) return HICGAT_EINVAL;
  hipLaunchKernelGGL(pairdist_fwd_kernel, dim3((N + 255) / 256, N), dim3(256), 0,
                     (hipStream_t)stream, coords, N, D, ldd);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_pairdist_bwd(const float *coords, const float *G, int N, int64_t ldg,
                                   float *dcoords, void *workspace, size_t workspace_bytes,
                                   hicgat_stream_t stream) {
  if (N < 0 || ldg < N) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!coords || !G || !dcoords || !workspace) return HICGAT_EINVAL;
  const PdLayout L = fused_layout(N, HICGAT_PD_SQUARE, false);
  if (workspace_bytes < L.total) return HICGAT_EINVAL;
  const int nb = pd_nb(N);
  const int64_t tiles = (int64_t)nb * nb;
  float4 *part = ws_at<float4>(workspace, L.part);
  double *mom = ws_at<double>(workspace, L.mom);
  if (t_is_vec(G, ldg, 0, nb))
    hipLaunchKernelGGL((pairdist_tile_kernel<MODE_FULL, true, KIND_MSE>), dim3(tiles), dim3(256), kTileLds,
                       (hipStream_t)stream, coords, G, N, ldg, (int64_t)0, (int64_t)0, nb, (int64_t)0, part, mom, 0.f);
  else
    hipLaunchKernelGGL((pairdist_tile_kernel<MODE_FULL, false, KIND_MSE>), dim3(tiles), dim3(256), 0,
                       (hipStream_t)stream, coords, G, N, ldg, (int64_t)0, (int64_t)0, nb, (int64_t)0, part, mom, 0.f);
  HICGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(pairdist_reduce_kernel, dim3((N + 63) / 64), dim3(1024), 0,
                     (hipStream_t)stream, part, N, nb, (int)MODE_FULL, (int64_t)0, tiles, 1.0f,
                     dcoords, nullptr, (int64_t)0, (int64_t)0, 0, nullptr, nullptr, 0, 0, nullptr);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_pairdist_mse_fused(const float *coords, const float *T, int N, int64_t ldt,
                                         int64_t t_row0, int64_t t_rows, int64_t t_col0,
                                         int64_t tile_begin, int64_t tile_end, int loss_kind,
                                         double *stats, float *loss, float *dcoords, void *workspace,
                                         size_t workspace_bytes, hicgat_stream_t stream) {
  if (N < 0 || !loss_kind_ok(loss_kind)) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!coords || !T || !stats || !workspace) return HICGAT_EINVAL;
  const PdLayout L = fused_layout(N, HICGAT_PD_TRI, false);
  if (workspace_bytes < L.total) return HICGAT_EINVAL;
  const int nb = pd_nb(N);
  if (!clamp_range(tile_begin, tile_end, hicgat_pairdist_num_tiles(N, HICGAT_PD_TRI))) return HICGAT_EINVAL;
  const int64_t nt = tile_end - tile_begin;
  if (nt > 0) {
    // the band must hold every row / column the tile range reads: rows of tile-rows I0..I1 and
    // columns from I0's diagonal tile on (tiles (I, J) have J >= I >= I0)
    const int64_t I0 = tri_row_host(tile_begin, nb), I1 = tri_row_host(tile_end - 1, nb);
    const int64_t need_r1 = std::min<int64_t>(N, (I1 + 1) * BT);
    if (t_row0 < 0 || t_col0 < 0 || t_row0 > I0 * BT || t_col0 > I0 * BT || t_row0 + t_rows < need_r1 ||
        ldt < (int64_t)N - t_col0)
      return HICGAT_EINVAL;
  }
  float4 *part = ws_at<float4>(workspace, L.part);
  double *mom = ws_at<double>(workspace, L.mom), *mpart = ws_at<double>(workspace, L.mpart);
  hipStream_t s = (hipStream_t)stream;
  if (nt > 0) {
    const bool vec = t_is_vec(T, ldt, t_col0, nb);
    with_kind(loss_kind, [&](auto kind_c) {
      constexpr int KD = decltype(kind_c)::value;
      if (vec)
        hipLaunchKernelGGL((pairdist_tile_kernel<MODE_SYM, true, KD>), dim3(nt), dim3(256), kTileLds, s, coords, T, N,
                           ldt, t_row0, t_col0, nb, tile_begin, part, mom, 0.f);
      else
        hipLaunchKernelGGL((pairdist_tile_kernel<MODE_SYM, false, KD>), dim3(nt), dim3(256), 0, s, coords, T, N, ldt,
                           t_row0, t_col0, nb, tile_begin, part, mom, 0.f);
    });
    HICGAT_CHECK_LAUNCH();
  }
  // row / column partials -> dcoords (when wanted) and, in the same launch, kMomBlocks blocks of
  // tile-moment partials; then one small launch: partials -> stats[0..6] -> mse / r / alpha / total
  const float scale = loss_scale(N, loss_kind);
  const int row_blocks = dcoords ? (N + 63) / 64 : 0;
  hipLaunchKernelGGL(pairdist_reduce_kernel, dim3(row_blocks + kMomBlocks), dim3(1024), 0, s, part, N, nb,
                     (int)MODE_SYM, tile_begin, tile_end, scale, dcoords, mom, tile_begin, tile_end, row_blocks, mpart,
                     nullptr, 0, 0, nullptr);
  HICGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(moments_finalize_kernel, dim3(1), dim3(64), 0, s, mpart, N, loss_kind, stats, loss);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_pairdist_finalize(int N, int loss_kind, double *stats, float *loss,
                                        hicgat_stream_t stream) {
  if (N <= 0 || !stats || !loss_kind_ok(loss_kind)) return HICGAT_EINVAL;
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, N, loss_kind,
                     stats, loss);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_pairdist_finalize_rows(int N, int loss_kind, double *stats, float *loss, const double *dc64,
                                             int row_begin, int row_end, float *dcoords, const float *cbuf,
                                             const int32_t *gidx, float *cglob, hicgat_stream_t stream) {
  if (N <= 0 || !stats || !loss_kind_ok(loss_kind)) return HICGAT_EINVAL;
  if (row_begin < 0 || row_end > N || row_begin > row_end) return HICGAT_EINVAL;
  const int64_t n3 = 3 * (int64_t)(row_end - row_begin);
  if (n3 > 0 && (!dc64 || !dcoords)) return HICGAT_EINVAL;
  if (cbuf && (!gidx || !cglob)) return HICGAT_EINVAL;
  const int64_t off = 3 * (int64_t)row_begin;
  const int64_t work = std::max<int64_t>(std::max<int64_t>(n3, cbuf ? 3 * (int64_t)N : 0), 1);
  hipLaunchKernelGGL(finalize_rows_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N,
                     loss_kind, stats, loss, n3 ? dc64 + off : nullptr, n3, n3 ? dcoords + off : nullptr, cbuf, gidx,
                     cglob);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

// background form: T = bg except at a sorted symmetric CSR support + the diagonal
extern "C" int hicgat_pairdist_mse_fused_support(const float *coords, const int32_t *cmap, int N, float background,
                                                 const int32_t *rowptr, const int32_t *col, const float *val,
                                                 const float *diag, int64_t tile_begin, int64_t tile_end,
                                                 int support_row_begin, int support_row_end, int loss_kind,
                                                 double *stats, float *loss, float *dcoords, double *dcoords64,
                                                 void *workspace, size_t workspace_bytes, hicgat_stream_t stream) {
  if (N < 0 || !loss_kind_ok(loss_kind)) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!coords || !rowptr || !col || !val || !diag || !stats || !workspace) return HICGAT_EINVAL;
  const PdLayout L = fused_layout(N, HICGAT_PD_TRI, true);
  if (workspace_bytes < L.total) return HICGAT_EINVAL;
  const int nb = pd_nb(N);
  const int64_t tiles = hicgat_pairdist_num_tiles(N, HICGAT_PD_TRI);
  int64_t s0 = support_row_begin, s1 = support_row_end;
  if (!clamp_range(tile_begin, tile_end, tiles) || !clamp_range(s0, s1, N)) return HICGAT_EINVAL;
  const int64_t nt = tile_end - tile_begin;
  const int64_t sblocks = (s1 - s0 + 3) / 4;
  float4 *part = ws_at<float4>(workspace, L.part), *corr = ws_at<float4>(workspace, L.corr);
  double *mom = ws_at<double>(workspace, L.mom), *mpart = ws_at<double>(workspace, L.mpart);
  double *smom = mom + (size_t)tile_end * 8;   // the support blocks' records (PdLayout)
  hipStream_t s = (hipStream_t)stream;
  // bulk: every pair i < j of the tile range at the background value (no T read); support: the
  // entries of rows [s0, s1) that differ, and those rows' diagonal
  // a rank's share (dcoords64: the sharded step): the support blocks ride in the tile launch (one
  // launch fewer on the critical path; at N = 20000 on one GPU the support pass needs the occupancy
  // of its own launch: 1.881 / 1.884 vs 1.875 / 1.877 ms per step, profiles/r04u_ab_single_gpu.txt)
  const bool ride = dcoords64 && nt > 0 && sblocks > 0;
  SupportArgs sa;
  if (ride) sa = SupportArgs{rowptr, col, val, diag, corr, smom, (int)s0, (int)s1, nt};
  // the whole triangle in one launch before a separate support launch (one GPU): the diagonal tiles
  // write the float4 copy of the coordinates the support pass gathers (19 -> 8 us at N = 20000)
  float4 *cpad = (!ride && !cmap && tile_begin == 0 && tile_end == tiles && sblocks > 0)
                     ? ws_at<float4>(workspace, L.cpad) : nullptr;
  with_kind(loss_kind, [&](auto kind_c) {
    constexpr int KD = decltype(kind_c)::value;
    if (ride)
      hipLaunchKernelGGL((pairdist_tile_kernel<MODE_SYM, false, KD, true, true>), dim3(nt + sblocks), dim3(256), 0, s,
                         coords, nullptr, N, (int64_t)0, (int64_t)0, (int64_t)0, nb, tile_begin, part, mom, background,
                         cmap, sa);
    else if (nt > 0)
      hipLaunchKernelGGL((pairdist_tile_kernel<MODE_SYM, false, KD, true>), dim3(nt), dim3(256), 0, s, coords,
                         nullptr, N, (int64_t)0, (int64_t)0, (int64_t)0, nb, tile_begin, part, mom, background, cmap,
                         SupportArgs{}, cpad);
    if (sblocks > 0 && !ride)
      hipLaunchKernelGGL(pairdist_support_kernel<KD>, dim3(sblocks), dim3(256), 0, s, coords, N, background, (int)s0,
                         (int)s1, rowptr, col, val, diag, corr, smom, cmap, cpad);
  });
  HICGAT_CHECK_LAUNCH();
  const float scale = loss_scale(N, loss_kind);
  const int row_blocks = (dcoords || dcoords64) ? (N + 63) / 64 : 0;
  // dcoords64: the caller all-reduces [stats | dcoords64] and finalizes (hicgat_pairdist_finalize_rows),
  // so a small share's moments go straight into stats[0..6] (stats[7..11] and loss are left alone)
  const bool one = dcoords64 && nt + sblocks <= kOneBlockMoments;
  hipLaunchKernelGGL(pairdist_reduce_kernel, dim3(row_blocks + (one ? 1 : kMomBlocks)), dim3(1024), 0, s, part, N, nb,
                     (int)MODE_SYM, tile_begin, tile_end, scale, dcoords, mom, tile_begin, tile_end + sblocks,
                     row_blocks, one ? stats : mpart, corr, (int)s0, (int)s1, dcoords64);
  HICGAT_CHECK_LAUNCH();
  if (!one) {
    hipLaunchKernelGGL(moments_finalize_kernel, dim3(1), dim3(64), 0, s, mpart, N, loss_kind, stats, loss);
    HICGAT_CHECK_LAUNCH();
  }
  return HICGAT_OK;
}

// moment-dependent losses: tile pass -> reduce -> finalize + combine.  T == NULL: the background form
// (rowptr / col / val / diag and background)
static int mloss_run(const float *coords, const float *T, int64_t ldt, int N, float background, const int32_t *rowptr,
                     const int32_t *col, const float *val, const float *diag, int mloss_kind, double alpha,
                     double *stats, float *loss, float *dcoords, void *workspace, size_t workspace_bytes,
                     hipStream_t s) {
  const bool support = T == nullptr;
  const PdLayout L = mloss_layout(N, support);
  if (workspace_bytes < L.total) return HICGAT_EINVAL;
  const int nb = pd_nb(N);
  const int64_t tiles = hicgat_pairdist_num_tiles(N, HICGAT_PD_TRI);
  const int64_t sblocks = support ? pd_support_blocks(N) : 0;
  float4 *part = ws_at<float4>(workspace, L.part), *rw = ws_at<float4>(workspace, L.rw);
  double *mom = ws_at<double>(workspace, L.mom), *mpart = ws_at<double>(workspace, L.mpart);
  double *csum = ws_at<double>(workspace, L.csum);
  float4 *corr = support ? ws_at<float4>(workspace, L.corr) : nullptr;
  float4 *cpad = support ? ws_at<float4>(workspace, L.cpad) : nullptr;
  if (support) {
    hipLaunchKernelGGL(pairdist_mloss_tile_kernel<true>, dim3(tiles), dim3(256), 0, s, coords, nullptr, N,
                       (int64_t)0, 0, nb, part, mom, background, cpad);
    HICGAT_CHECK_LAUNCH();
    // the support's change of R_i and of sum (d-t)^2, sum dt, sum t, sum t^2, and sum T_ii^2: the combined
    // loss's support pass as it is (W has no t in it: the bulk pass alone gives it)
    hipLaunchKernelGGL(pairdist_support_kernel<KIND_COMBINED>, dim3(sblocks), dim3(256), 0, s, coords, N, background,
                       0, N, rowptr, col, val, diag, corr, mom + (size_t)tiles * 8, nullptr, cpad);
  } else {
    hipLaunchKernelGGL(pairdist_mloss_tile_kernel<false>, dim3(tiles), dim3(256), 0, s, coords, T, N, ldt,
                       t_is_vec(T, ldt, 0, nb) ? 1 : 0, nb, part, mom, 0.f, nullptr);
  }
  HICGAT_CHECK_LAUNCH();
  const int row_blocks = (N + 63) / 64;
  hipLaunchKernelGGL(pairdist_mloss_reduce_kernel, dim3(row_blocks + kMomBlocks + 1), dim3(1024), 0, s, part, N, nb,
                     rw, mom, tiles, tiles + sblocks, row_blocks, mpart, corr, coords, support ? diag : nullptr,
                     csum);
  HICGAT_CHECK_LAUNCH();
  hipLaunchKernelGGL(pairdist_mloss_finalize_kernel, dim3((N + 255) / 256), dim3(256), 0, s, mpart, csum, rw, coords,
                     N, mloss_kind, alpha, stats, loss, dcoords);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

static bool mloss_kind_ok(int k) { return k == MLOSS_PEARSON || k == MLOSS_RMSE || k == MLOSS_SI_MSE; }

extern "C" int hicgat_pairdist_moment_loss(const float *coords, const float *T, int N, int64_t ldt, int mloss_kind,
                                           double alpha, double *stats, float *loss, float *dcoords,
                                           void *workspace, size_t workspace_bytes, hicgat_stream_t stream) {
  if (N < 0 || !mloss_kind_ok(mloss_kind) || !(alpha == alpha)) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!coords || !T || !stats || !workspace || ldt < N) return HICGAT_EINVAL;
  return mloss_run(coords, T, ldt, N, 0.f, nullptr, nullptr, nullptr, nullptr, mloss_kind, alpha, stats, loss,
                   dcoords, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int hicgat_pairdist_moment_loss_support(const float *coords, int N, float background,
                                                   const int32_t *rowptr, const int32_t *col, const float *val,
                                                   const float *diag, int mloss_kind, double alpha, double *stats,
                                                   float *loss, float *dcoords, void *workspace,
                                                   size_t workspace_bytes, hicgat_stream_t stream) {
  if (N < 0 || !mloss_kind_ok(mloss_kind) || !(alpha == alpha)) return HICGAT_EINVAL;
  if (N == 0) return HICGAT_OK;
  if (!coords || !rowptr || !col || !val || !diag || !stats || !workspace) return HICGAT_EINVAL;
  return mloss_run(coords, nullptr, 0, N, background, rowptr, col, val, diag, mloss_kind, alpha, stats, loss, dcoords,
                   workspace, workspace_bytes, (hipStream_t)stream);
}
