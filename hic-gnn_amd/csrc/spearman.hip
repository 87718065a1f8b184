// Exact Spearman correlation on the device (a11, per-step dSCC): a stable LSD radix sort of
// (32-bit key, 32-bit payload) pairs and one tie-aware reduction over the sorted arrays.
//
//   key     = the order-preserving image of a float's bits (-0 canonicalised to +0, so they tie as in
//             scipy; bits are compared, never floats, so denormals stay distinct)
//   payload = the truth's doubled average rank of that element (scoring) or the element's index
//             (hicgat_avg_rank2, which prepares those ranks)
//
// Four 8-bit passes, each = per-tile digit histogram -> scan of the [digit][tile] table -> stable
// scatter.  Order between tiles comes from kernel boundaries only: no workgroup waits on another.
// A pass whose digit is the same for every key is skipped on the device: the global digit counts
// of all four passes are taken in one read before the first pass, a one-block kernel turns them
// into a plan (skip flags + which ping-pong buffer each pass reads), and every later kernel reads
// the plan.  Integer atomics only (LDS histograms, the global digit counts, the NaN flag); every
// fp64 sum runs in a fixed order, so two runs give the same bits.
//
// Tie-aware reduction: a tie group at sorted positions s..e has average rank (s + e)/2 + 1; with
// doubled, centred ranks a = 2 R_truth - (M+1), b = 2 R_pred - (M+1) = s + e + 1 - M (integers,
// |.| <= M) rho = sum(ab) / sqrt(sum(a^2) sum(b^2)).  Per tile the groups that lie strictly inside
// it are summed there (sum of a in int64, times b once, in fp64); the runs that touch a tile's ends
// are handed to the stitch kernel as records (key, count, sum a), which joins a group over any
// number of tiles.
#include "common.hpp"

namespace hicgat {
namespace {

constexpr int RK_THREADS = 256;                 // 4 waves
constexpr int RK_KPT = 16;                      // keys per thread
constexpr int RK_TILE = RK_THREADS * RK_KPT;    // 4096 keys per tile
constexpr int RK_WAVE_KEYS = 64 * RK_KPT;       // a wave's contiguous share of the tile
constexpr int RK_GHIST_BLOCKS = 1024;

struct RankPlan {
  uint32_t skip[4];   // pass p is skipped (its digit is constant over all keys)
  uint32_t src[4];    // ping-pong buffer pass p reads
  uint32_t fin;       // buffer that holds the sorted arrays
  uint32_t pad[7];
};

// The caller's workspace, carved (every part 256-B aligned).
struct RankWs {
  uint32_t *key[2], *val[2];
  uint32_t *table;     // [256][tiles] digit counts -> exclusive offsets of the running pass
  uint32_t *ctrl;      // [4][256] global digit counts, then the NaN flag word (zeroed per call)
  RankPlan *plan;
  uint32_t *first, *last, *lead, *trail, *lead_r2, *trail_r2;   // per tile
  long long *lead_a, *trail_a;                                  // per tile
  double *partial;                                              // [tiles][3]: sum ab, sum b^2, groups
  size_t total;
};
constexpr size_t RK_CTRL_WORDS = 4 * 256 + 64;

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

int64_t rank_tiles(int64_t M) { return (M + RK_TILE - 1) / RK_TILE; }

RankWs rank_carve(void *ws, int64_t M) {
  RankWs w;
  char *p = static_cast<char *>(ws);
  size_t o = 0;
  const size_t tiles = (size_t)rank_tiles(M);
  auto take = [&](size_t bytes) {
    char *q = p + o;
    o += up256(bytes);
    return q;
  };
  for (int b = 0; b < 2; ++b) w.key[b] = reinterpret_cast<uint32_t *>(take((size_t)M * 4));
  for (int b = 0; b < 2; ++b) w.val[b] = reinterpret_cast<uint32_t *>(take((size_t)M * 4));
  w.table = reinterpret_cast<uint32_t *>(take(tiles * 256 * 4));
  w.ctrl = reinterpret_cast<uint32_t *>(take(RK_CTRL_WORDS * 4));
  w.plan = reinterpret_cast<RankPlan *>(take(sizeof(RankPlan)));
  w.first = reinterpret_cast<uint32_t *>(take(tiles * 4));
  w.last = reinterpret_cast<uint32_t *>(take(tiles * 4));
  w.lead = reinterpret_cast<uint32_t *>(take(tiles * 4));
  w.trail = reinterpret_cast<uint32_t *>(take(tiles * 4));
  w.lead_r2 = reinterpret_cast<uint32_t *>(take(tiles * 4));
  w.trail_r2 = reinterpret_cast<uint32_t *>(take(tiles * 4));
  w.lead_a = reinterpret_cast<long long *>(take(tiles * 8));
  w.trail_a = reinterpret_cast<long long *>(take(tiles * 8));
  w.partial = reinterpret_cast<double *>(take(tiles * 3 * 8));
  w.total = o;
  return w;
}

bool rank_supported(int64_t M) { return M < ((int64_t)1 << 31); }
bool misaligned(const void *ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) != 0; }

// ---- keys -------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t float_key(float f, bool &is_nan) {
  uint32_t b = __float_as_uint(f);
  is_nan = (b & 0x7fffffffu) > 0x7f800000u;
  if (b == 0x80000000u) b = 0u;                        // -0 ties with +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Pair (i, j), i < j, number x of the block row r: rows r and N-2-r together hold N pairs, so a
// grid of ceil((N-1)/2) block rows of N threads covers the upper triangle with no idle thread.
__device__ __forceinline__ bool triu_pair(int N, int r, int x, int &i, int &j) {
  const int len = N - 1 - r;
  if (x < len) {
    i = r;
    j = r + 1 + x;
    return true;
  }
  const int r2 = N - 2 - r, x2 = x - len;
  if (r2 == r || x2 > r) return false;
  i = r2;
  j = r2 + 1 + x2;
  return true;
}
// k of torch.triu_indices(N, N, 1) for (i, j)
__device__ __forceinline__ int64_t triu_index(int N, int i, int j) {
  return (int64_t)i * N - ((int64_t)i * (i + 1)) / 2 + (j - i - 1);
}

__global__ __launch_bounds__(256) void rank_triu_gather_kernel(const float *__restrict__ T, int N, int64_t ld,
                                                               float *__restrict__ v) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  int i, j;
  if (x >= N || !triu_pair(N, blockIdx.y, x, i, j)) return;
  v[triu_index(N, i, j)] = T[(int64_t)i * ld + j];
}

// payload = rank2[k] (scoring) or k (rank2 == nullptr: preparing the ranks)
__global__ __launch_bounds__(256) void rank_keygen_vec_kernel(const float *__restrict__ v, int64_t M,
                                                              const uint32_t *__restrict__ rank2,
                                                              uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                              uint32_t *__restrict__ nan_flag) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= M) return;
  bool is_nan;
  key[k] = float_key(v[k], is_nan);
  val[k] = rank2 ? rank2[k] : (uint32_t)k;
  if (is_nan) atomicOr(nan_flag, 1u);
}

// The per-step form: the distance of pair k with the expression of pairdist_fwd_kernel (same bits
// as ops.pairwise_dist), straight into key / payload; D is never stored.
__global__ __launch_bounds__(256) void rank_keygen_coords_kernel(const float *__restrict__ coords, int N,
                                                                 const uint32_t *__restrict__ rank2,
                                                                 uint32_t *__restrict__ key,
                                                                 uint32_t *__restrict__ val,
                                                                 uint32_t *__restrict__ nan_flag) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  int i, j;
  if (x >= N || !triu_pair(N, blockIdx.y, x, i, j)) return;
  const float dx = coords[3 * (size_t)i] - coords[3 * (size_t)j],
              dy = coords[3 * (size_t)i + 1] - coords[3 * (size_t)j + 1],
              dz = coords[3 * (size_t)i + 2] - coords[3 * (size_t)j + 2];
  const float d = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
  const int64_t k = triu_index(N, i, j);
  bool is_nan;
  key[k] = float_key(d, is_nan);
  val[k] = rank2[k];
  if (is_nan) atomicOr(nan_flag, 1u);
}

// ---- the radix passes -------------------------------------------------------------------------

// Global counts of all four digits in one read of the keys.
__global__ __launch_bounds__(RK_THREADS) void rank_ghist_kernel(const uint32_t *__restrict__ key, int64_t M,
                                                                uint32_t *__restrict__ totals) {
  __shared__ uint32_t h[4 * 256];
  for (int q = threadIdx.x; q < 4 * 256; q += RK_THREADS) h[q] = 0;
  __syncthreads();
  for (int64_t k = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x; k < M; k += (int64_t)gridDim.x * RK_THREADS) {
    const uint32_t x = key[k];
    atomicAdd(&h[x & 255u], 1u);
    atomicAdd(&h[256 + ((x >> 8) & 255u)], 1u);
    atomicAdd(&h[512 + ((x >> 16) & 255u)], 1u);
    atomicAdd(&h[768 + (x >> 24)], 1u);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < 4 * 256; q += RK_THREADS)
    if (h[q]) atomicAdd(&totals[q], h[q]);
}

__global__ __launch_bounds__(RK_THREADS) void rank_plan_kernel(const uint32_t *__restrict__ totals, uint32_t M,
                                                               RankPlan *__restrict__ plan) {
  __shared__ uint32_t sk[4];
  if (threadIdx.x < 4) sk[threadIdx.x] = 0;
  __syncthreads();
  for (int p = 0; p < 4; ++p)
    if (totals[p * 256 + threadIdx.x] == M) atomicOr(&sk[p], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t parity = 0;
    for (int p = 0; p < 4; ++p) {
      plan->skip[p] = sk[p];
      plan->src[p] = parity;
      if (!sk[p]) parity ^= 1u;
    }
    plan->fin = parity;
  }
}

__global__ __launch_bounds__(RK_THREADS) void rank_hist_kernel(const uint32_t *__restrict__ key0,
                                                               const uint32_t *__restrict__ key1, int64_t M,
                                                               int tiles, int pass, const RankPlan *__restrict__ plan,
                                                               uint32_t *__restrict__ table) {
  if (plan->skip[pass]) return;
  const uint32_t *__restrict__ key = plan->src[pass] ? key1 : key0;
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t p0 = (int64_t)blockIdx.x * RK_TILE;
  const int shift = pass * 8;
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    const int64_t k = p0 + j * RK_THREADS + threadIdx.x;
    if (k < M) atomicAdd(&h[(key[k] >> shift) & 255u], 1u);
  }
  __syncthreads();
  table[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// Inclusive scan over the block's 256 threads in LDS (Hillis-Steele, double buffered).  `r` is the
// thread's place in the scan order.  The result of place q is left in buf[q]; the caller syncs
// before it reuses buf.
template <class T, class Op>
__device__ __forceinline__ T block_scan_incl(T v, T *buf, Op op, int r) {
  int cur = 0;
  buf[r] = v;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < RK_THREADS; o <<= 1) {
    T a = buf[cur * RK_THREADS + r];
    if (r >= o) a = op(buf[cur * RK_THREADS + r - o], a);
    buf[(cur ^ 1) * RK_THREADS + r] = a;
    cur ^= 1;
    __syncthreads();
  }
  return buf[r];   // eight steps: cur is 0 again
}

struct AddU32 {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
// "the later one if it is set": nearest start to the left / nearest end to the right
struct LaterInt {
  __device__ int operator()(int l, int r) const { return r >= 0 ? r : l; }
};

// Row d of the [digit][tile] table -> exclusive offsets: keys of smaller digits first, then the
// same digit's keys of earlier tiles.  One block per digit.
__global__ __launch_bounds__(RK_THREADS) void rank_scan_kernel(uint32_t *__restrict__ table, int tiles, int pass,
                                                               const RankPlan *__restrict__ plan,
                                                               const uint32_t *__restrict__ totals) {
  if (plan->skip[pass]) return;
  __shared__ uint32_t buf[2 * RK_THREADS];
  const int d = blockIdx.x, tid = threadIdx.x;
  block_scan_incl<uint32_t>(tid < d ? totals[pass * 256 + tid] : 0u, buf, AddU32(), tid);
  uint32_t carry = buf[RK_THREADS - 1];
  __syncthreads();
  uint32_t *__restrict__ row = table + (size_t)d * tiles;
  for (int c0 = 0; c0 < tiles; c0 += 4 * RK_THREADS) {
    uint32_t x[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = c0 + tid * 4 + q;
      x[q] = t < tiles ? row[t] : 0u;
      s += x[q];
    }
    const uint32_t incl = block_scan_incl<uint32_t>(s, buf, AddU32(), tid);
    const uint32_t chunk = buf[RK_THREADS - 1];
    __syncthreads();
    uint32_t run = carry + incl - s;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = c0 + tid * 4 + q;
      if (t < tiles) row[t] = run;
      run += x[q];
    }
    carry += chunk;
  }
}

// Stable scatter of one tile.  Wave w owns keys [w * 1024, (w+1) * 1024) of the tile, item j of lane
// l at w * 1024 + j * 64 + l, so (wave, item, lane) order is element order.  Per item the lanes of
// equal digit find each other with eight ballots; the lowest of them takes the wave's running count
// of that digit from LDS (the wave's own row: no other wave touches it) and adds the group's size.
__global__ __launch_bounds__(RK_THREADS) void rank_scatter_kernel(uint32_t *__restrict__ key0,
                                                                  uint32_t *__restrict__ key1,
                                                                  uint32_t *__restrict__ val0,
                                                                  uint32_t *__restrict__ val1, int64_t M, int tiles,
                                                                  int pass, const RankPlan *__restrict__ plan,
                                                                  const uint32_t *__restrict__ table) {
  if (plan->skip[pass]) return;
  const bool from1 = plan->src[pass] != 0;
  const uint32_t *__restrict__ skey = from1 ? key1 : key0;
  const uint32_t *__restrict__ sval = from1 ? val1 : val0;
  uint32_t *__restrict__ dkey = from1 ? key0 : key1;
  uint32_t *__restrict__ dval = from1 ? val0 : val1;

  __shared__ uint32_t cnt[4][256];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q][tid] = 0;
  __syncthreads();

  const int64_t base = (int64_t)blockIdx.x * RK_TILE + (int64_t)w * RK_WAVE_KEYS + lane;
  const int shift = pass * 8;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t k[RK_KPT], v[RK_KPT], rk[RK_KPT];
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    const int64_t idx = base + j * 64;
    const bool valid = idx < M;
    k[j] = valid ? skey[idx] : 0u;
    v[j] = valid ? sval[idx] : 0u;
  }
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    const bool valid = base + j * 64 < M;
    const uint32_t d = (k[j] >> shift) & 255u;
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    if (!valid) m = 0ull;
    const int before = __popcll(m & below);
    uint32_t pre = 0;
    if (valid && before == 0) pre = atomicAdd(&cnt[w][d], (uint32_t)__popcll(m));
    const int leader = m ? __ffsll((long long)m) - 1 : lane;
    pre = __shfl(pre, leader);
    rk[j] = pre + before;
  }
  __syncthreads();
  {  // digit tid: the tile's offset in the output, then each wave's start inside the tile's run
    uint32_t run = table[(size_t)tid * tiles + blockIdx.x];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c = cnt[q][tid];
      cnt[q][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    if (base + j * 64 < M) {
      const uint32_t d = (k[j] >> shift) & 255u;
      const int64_t pos = (int64_t)cnt[w][d] + rk[j];
      if (pos < M) {
        dkey[pos] = k[j];
        dval[pos] = v[j];
      }
    }
  }
}

// ---- the tie-aware reduction ------------------------------------------------------------------

// Scan element of the in-tile pass: the sum of a so far, the latest group start and the sum of a
// before that start.
struct Seg {
  long long sum, pstart;
  int start, pad;
};
struct SegOp {
  __device__ Seg operator()(const Seg &l, const Seg &r) const {
    Seg o;
    o.sum = l.sum + r.sum;
    o.pad = 0;
    if (r.start >= 0) {
      o.start = r.start;
      o.pstart = l.sum + r.pstart;
    } else {
      o.start = l.start;
      o.pstart = l.pstart;
    }
    return o;
  }
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A thread's 16 consecutive sorted keys (and payloads) of tile `t`, with the neighbours' keys.
struct TileSlice {
  uint32_t k[RK_KPT], v[RK_KPT];
  uint32_t prev, next;
  int i0, nv, n;
  int64_t p0;
};
template <bool WITH_VAL>
__device__ __forceinline__ void load_slice(TileSlice &s, const uint32_t *__restrict__ key,
                                           const uint32_t *__restrict__ val, int64_t M, int t) {
  s.p0 = (int64_t)t * RK_TILE;
  const int64_t left = M - s.p0;
  s.n = left < RK_TILE ? (int)left : RK_TILE;
  s.i0 = threadIdx.x * RK_KPT;
  s.nv = s.n - s.i0;
  s.nv = s.nv < 0 ? 0 : (s.nv > RK_KPT ? RK_KPT : s.nv);
  if (s.nv == RK_KPT) {
    const uint4 *kq = reinterpret_cast<const uint4 *>(key + s.p0 + s.i0);
#pragma unroll
    for (int q = 0; q < RK_KPT / 4; ++q) {
      const uint4 a = kq[q];
      s.k[4 * q] = a.x, s.k[4 * q + 1] = a.y, s.k[4 * q + 2] = a.z, s.k[4 * q + 3] = a.w;
    }
    if (WITH_VAL) {
      const uint4 *vq = reinterpret_cast<const uint4 *>(val + s.p0 + s.i0);
#pragma unroll
      for (int q = 0; q < RK_KPT / 4; ++q) {
        const uint4 a = vq[q];
        s.v[4 * q] = a.x, s.v[4 * q + 1] = a.y, s.v[4 * q + 2] = a.z, s.v[4 * q + 3] = a.w;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < RK_KPT; ++j) {
      s.k[j] = j < s.nv ? key[s.p0 + s.i0 + j] : 0u;
      s.v[j] = (WITH_VAL && j < s.nv) ? val[s.p0 + s.i0 + j] : 0u;
    }
  }
  s.prev = (s.i0 > 0 && s.nv > 0) ? key[s.p0 + s.i0 - 1] : 0u;
  s.next = (s.i0 + RK_KPT < s.n) ? key[s.p0 + s.i0 + RK_KPT] : 0u;
}
__device__ __forceinline__ bool is_start(const TileSlice &s, int j) {
  return (s.i0 + j == 0) || s.k[j] != (j ? s.k[j ? j - 1 : 0] : s.prev);
}
__device__ __forceinline__ bool is_end(const TileSlice &s, int j) {
  return (s.i0 + j == s.n - 1) || s.k[j] != (j < RK_KPT - 1 ? s.k[j < RK_KPT - 1 ? j + 1 : j] : s.next);
}

// Per tile of the sorted arrays: the groups strictly inside it into partial[t], the runs at its two
// ends into the records.
__global__ __launch_bounds__(RK_THREADS) void rank_tile_reduce_kernel(
    const uint32_t *__restrict__ key0, const uint32_t *__restrict__ key1, const uint32_t *__restrict__ val0,
    const uint32_t *__restrict__ val1, int64_t M, const RankPlan *__restrict__ plan, uint32_t *__restrict__ first,
    uint32_t *__restrict__ last, uint32_t *__restrict__ lead, uint32_t *__restrict__ trail,
    long long *__restrict__ lead_a, long long *__restrict__ trail_a, double *__restrict__ partial) {
  const bool fin = plan->fin != 0;
  const uint32_t *__restrict__ key = fin ? key1 : key0;
  const uint32_t *__restrict__ val = fin ? val1 : val0;
  __shared__ Seg buf[2 * RK_THREADS];
  __shared__ double red[3][4];
  const int t = blockIdx.x, tid = threadIdx.x;
  TileSlice s;
  load_slice<true>(s, key, val, M, t);
  const long long centre = (long long)M + 1;

  Seg agg{0, 0, -1, 0};
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    if (j < s.nv) {
      if (is_start(s, j)) {
        agg.start = s.i0 + j;
        agg.pstart = agg.sum;
      }
      agg.sum += (long long)s.v[j] - centre;
    }
  }
  block_scan_incl<Seg>(agg, buf, SegOp(), tid);
  Seg cur = tid ? buf[tid - 1] : Seg{0, 0, -1, 0};

  double ab = 0.0, bb = 0.0, ng = 0.0;
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    if (j < s.nv) {
      const int i = s.i0 + j;
      if (is_start(s, j)) {
        cur.start = i;
        cur.pstart = cur.sum;
      }
      cur.sum += (long long)s.v[j] - centre;
      if (i == 0) first[t] = s.k[j];
      if (i == s.n - 1) last[t] = s.k[j];
      if (is_end(s, j)) {
        const int st = cur.start;
        const long long sum_a = cur.sum - cur.pstart;
        const int cnt = i - st + 1;
        if (st == 0 || i == s.n - 1) {
          if (st == 0) lead[t] = (uint32_t)cnt, lead_a[t] = sum_a;
          if (i == s.n - 1) trail[t] = (uint32_t)cnt, trail_a[t] = sum_a;
        } else {
          const double b = (double)(2 * s.p0 + st + i + 1 - (long long)M);
          ab += b * (double)sum_a;
          bb += (double)cnt * (b * b);
          ng += 1.0;
        }
      }
    }
  }
  ab = wave_sum_f64(ab), bb = wave_sum_f64(bb), ng = wave_sum_f64(ng);
  if ((tid & 63) == 0) red[0][tid >> 6] = ab, red[1][tid >> 6] = bb, red[2][tid >> 6] = ng;
  __syncthreads();
  if (tid < 3) partial[(size_t)t * 3 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// One thread per tile: the groups that BEGIN in the tile's end runs, followed over as many tiles as
// they span, are added to the tile's partial.  The doubled ranks of the end runs go to lead_r2 /
// trail_r2 for hicgat_avg_rank2's write pass.  No thread waits on another: each group has one owner
// (the tile it starts in), who reads records that the previous kernel completed.
__global__ __launch_bounds__(RK_THREADS) void rank_stitch_kernel(
    int64_t M, int tiles, const uint32_t *__restrict__ first, const uint32_t *__restrict__ last,
    const uint32_t *__restrict__ lead, const uint32_t *__restrict__ trail, const long long *__restrict__ lead_a,
    const long long *__restrict__ trail_a, uint32_t *__restrict__ lead_r2, uint32_t *__restrict__ trail_r2,
    double *__restrict__ partial) {
  const int t = blockIdx.x * RK_THREADS + threadIdx.x;
  if (t >= tiles) return;
  const int64_t p0 = (int64_t)t * RK_TILE;
  const int64_t left = M - p0;
  const uint32_t n = left < RK_TILE ? (uint32_t)left : (uint32_t)RK_TILE;
  double ab = partial[(size_t)t * 3], bb = partial[(size_t)t * 3 + 1], ng = partial[(size_t)t * 3 + 2];
  const bool all_same = lead[t] == n;
  const bool lead_starts = t == 0 || last[t - 1] != first[t];

  for (int which = 0; which < 2; ++which) {
    // which 0: the leading run, if its group starts here; 1: the trailing run of a tile with two runs
    if (which == 0 ? !lead_starts : all_same) continue;
    const uint32_t gkey = which == 0 ? first[t] : last[t];
    int64_t cnt = which == 0 ? lead[t] : trail[t];
    long long sum_a = which == 0 ? lead_a[t] : trail_a[t];
    const int64_t st = which == 0 ? p0 : p0 + n - cnt;
    int u = t + 1;
    if (which == 1 || all_same) {
      while (u < tiles && first[u] == gkey) {
        const int64_t lu = M - (int64_t)u * RK_TILE;
        const uint32_t nu = lu < RK_TILE ? (uint32_t)lu : (uint32_t)RK_TILE;
        cnt += lead[u];
        sum_a += lead_a[u];
        const bool full = lead[u] == nu;
        ++u;
        if (!full) break;
      }
    }
    const int64_t en = st + cnt - 1;
    const double b = (double)(st + en + 1 - M);
    ab += b * (double)sum_a;
    bb += (double)cnt * (b * b);
    ng += 1.0;
    const uint32_t r2 = (uint32_t)(st + en + 2);
    if (which == 0) lead_r2[t] = r2;
    else trail_r2[t] = r2;
    for (int q = t + 1; q < u; ++q) lead_r2[q] = r2;
  }
  partial[(size_t)t * 3] = ab;
  partial[(size_t)t * 3 + 1] = bb;
  partial[(size_t)t * 3 + 2] = ng;
}

// hicgat_avg_rank2's write pass: rank2[index] = s + e + 2 of the element's tie group.
__global__ __launch_bounds__(RK_THREADS) void rank_write_kernel(
    const uint32_t *__restrict__ key0, const uint32_t *__restrict__ key1, const uint32_t *__restrict__ val0,
    const uint32_t *__restrict__ val1, int64_t M, const RankPlan *__restrict__ plan,
    const uint32_t *__restrict__ lead_r2, const uint32_t *__restrict__ trail_r2, uint32_t *__restrict__ rank2) {
  const bool fin = plan->fin != 0;
  const uint32_t *__restrict__ key = fin ? key1 : key0;
  const uint32_t *__restrict__ val = fin ? val1 : val0;
  __shared__ int buf[2 * RK_THREADS];
  const int t = blockIdx.x, tid = threadIdx.x;
  TileSlice s;
  load_slice<true>(s, key, val, M, t);

  int a_start = -1, a_end = -1;   // the thread's last start, its first end
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    if (j < s.nv) {
      if (is_start(s, j)) a_start = s.i0 + j;
      if (is_end(s, j) && a_end < 0) a_end = s.i0 + j;
    }
  }
  block_scan_incl<int>(a_start, buf, LaterInt(), tid);
  int cs = tid ? buf[tid - 1] : -1;
  __syncthreads();
  const int r = RK_THREADS - 1 - tid;             // ends: scanned from the right
  block_scan_incl<int>(a_end, buf, LaterInt(), r);
  int ce = r ? buf[r - 1] : -1;

  int e[RK_KPT];
#pragma unroll
  for (int j = RK_KPT - 1; j >= 0; --j) {
    if (j < s.nv && is_end(s, j)) ce = s.i0 + j;
    e[j] = ce;
  }
  const uint32_t lr2 = lead_r2[t], tr2 = trail_r2[t];
#pragma unroll
  for (int j = 0; j < RK_KPT; ++j) {
    if (j < s.nv) {
      if (is_start(s, j)) cs = s.i0 + j;
      const uint32_t r2 = cs == 0 ? lr2 : (e[j] == s.n - 1 ? tr2 : (uint32_t)(2 * s.p0 + cs + e[j] + 2));
      if (s.v[j] < M) rank2[s.v[j]] = r2;
    }
  }
}

// Sum of the tiles' partials in a fixed order (thread q: tiles q, q + 256, ...; then a fixed tree).
__device__ __forceinline__ void sum_partials(const double *__restrict__ partial, int tiles, double (&tot)[3],
                                             double (*red)[4]) {
  double acc[3] = {0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < tiles; t += RK_THREADS)
    for (int c = 0; c < 3; ++c) acc[c] += partial[(size_t)t * 3 + c];
  for (int c = 0; c < 3; ++c) acc[c] = wave_sum_f64(acc[c]);
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) red[c][threadIdx.x >> 6] = acc[c];
  __syncthreads();
  for (int c = 0; c < 3; ++c) tot[c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
}

// side_stats = (sum a^2, tie groups, NaN flag, M) of a prepared side
__global__ __launch_bounds__(RK_THREADS) void rank_side_stats_kernel(const double *__restrict__ partial, int tiles,
                                                                     int64_t M, const uint32_t *__restrict__ nan_flag,
                                                                     double *__restrict__ side_stats) {
  __shared__ double red[3][4];
  double tot[3];
  sum_partials(partial, tiles, tot, red);
  if (threadIdx.x == 0) {
    side_stats[0] = tot[1];
    side_stats[1] = tot[2];
    side_stats[2] = *nan_flag ? 1.0 : 0.0;
    side_stats[3] = (double)M;
  }
}

// out = (rho, sum b^2, tie groups of the scored side, NaN flag); rho = NaN for a NaN input, a
// constant side (denominator 0) or M < 2, as scipy.stats.spearmanr returns.
__global__ __launch_bounds__(RK_THREADS) void rank_finalize_kernel(const double *__restrict__ partial, int tiles,
                                                                   int64_t M, const uint32_t *__restrict__ nan_flag,
                                                                   const double *__restrict__ side_stats,
                                                                   double *__restrict__ out) {
  __shared__ double red[3][4];
  double tot[3];
  sum_partials(partial, tiles, tot, red);
  if (threadIdx.x == 0) {
    const bool nan_in = *nan_flag != 0 || side_stats[2] != 0.0;
    const double den = sqrt_rn_f64(side_stats[0]) * sqrt_rn_f64(tot[1]);
    double rho = fmin(fmax(tot[0] / den, -1.0), 1.0);
    if (nan_in || M < 2 || !(den > 0.0)) rho = __longlong_as_double(0x7ff8000000000000ll);
    out[0] = rho;
    out[1] = tot[1];
    out[2] = tot[2];
    out[3] = nan_in ? 1.0 : 0.0;
  }
}

// Everything after the keys are in buffer 0: digit counts, plan, four passes, tile reduction, stitch.
int rank_sort_reduce(const RankWs &w, int64_t M, hipStream_t s) {
  const int tiles = (int)rank_tiles(M);
  const dim3 blk(RK_THREADS);
  uint32_t *totals = w.ctrl;
  hipLaunchKernelGGL(rank_ghist_kernel, dim3(tiles < RK_GHIST_BLOCKS ? tiles : RK_GHIST_BLOCKS), blk, 0, s, w.key[0], M,
                     totals);
  hipLaunchKernelGGL(rank_plan_kernel, dim3(1), blk, 0, s, totals, (uint32_t)M, w.plan);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(rank_hist_kernel, dim3(tiles), blk, 0, s, w.key[0], w.key[1], M, tiles, pass, w.plan, w.table);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(256), blk, 0, s, w.table, tiles, pass, w.plan, totals);
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(tiles), blk, 0, s, w.key[0], w.key[1], w.val[0], w.val[1], M, tiles,
                       pass, w.plan, w.table);
  }
  hipLaunchKernelGGL(rank_tile_reduce_kernel, dim3(tiles), blk, 0, s, w.key[0], w.key[1], w.val[0], w.val[1], M, w.plan,
                     w.first, w.last, w.lead, w.trail, w.lead_a, w.trail_a, w.partial);
  hipLaunchKernelGGL(rank_stitch_kernel, dim3((tiles + RK_THREADS - 1) / RK_THREADS), blk, 0, s, M, tiles, w.first,
                     w.last, w.lead, w.trail, w.lead_a, w.trail_a, w.lead_r2, w.trail_r2, w.partial);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

int rank_begin(const RankWs &w, hipStream_t s) {
  return hipMemsetAsync(w.ctrl, 0, RK_CTRL_WORDS * 4, s) == hipSuccess ? HICGAT_OK : HICGAT_ELAUNCH;
}

dim3 triu_grid(int N) { return dim3((N + 255) / 256, (N - 1 + 1) / 2); }

// size and workspace checks shared by the entry points (unsupported sizes first: no pointer of a
// refused size is looked at)
int rank_check(int64_t M, const void *ws, size_t ws_bytes) {
  if (!rank_supported(M)) return HICGAT_EUNSUPPORTED;
  if (M < 1 || !ws || misaligned(ws, 256)) return HICGAT_EINVAL;
  if (ws_bytes < hicgat_rank_workspace_bytes(M)) return HICGAT_EINVAL;
  return HICGAT_OK;
}

}  // namespace
}  // namespace hicgat

using namespace hicgat;

extern "C" int hicgat_rank_tile(void) { return RK_TILE; }

extern "C" size_t hicgat_rank_workspace_bytes(int64_t M) {
  if (M < 1 || !rank_supported(M)) return 0;
  return rank_carve(nullptr, M).total;
}

extern "C" int hicgat_triu_gather(const float *T, int N, int64_t ld, float *v, hicgat_stream_t stream) {
  if (N > 65536) return HICGAT_EUNSUPPORTED;
  if (N < 2 || !T || !v || ld < N) return HICGAT_EINVAL;
  hipLaunchKernelGGL(rank_triu_gather_kernel, triu_grid(N), dim3(256), 0, (hipStream_t)stream, T, N, ld, v);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_avg_rank2(const float *v, int64_t M, uint32_t *rank2, double *side_stats, void *ws,
                                size_t ws_bytes, hicgat_stream_t stream) {
  const int rc = rank_check(M, ws, ws_bytes);
  if (rc != HICGAT_OK) return rc;
  if (!v || !rank2 || !side_stats || misaligned(side_stats, 8)) return HICGAT_EINVAL;
  const RankWs w = rank_carve(ws, M);
  hipStream_t s = (hipStream_t)stream;
  if (rank_begin(w, s) != HICGAT_OK) return HICGAT_ELAUNCH;
  uint32_t *nan_flag = w.ctrl + 4 * 256;
  hipLaunchKernelGGL(rank_keygen_vec_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, v, M,
                     (const uint32_t *)nullptr, w.key[0], w.val[0], nan_flag);
  const int rs = rank_sort_reduce(w, M, s);
  if (rs != HICGAT_OK) return rs;
  const int tiles = (int)rank_tiles(M);
  hipLaunchKernelGGL(rank_write_kernel, dim3(tiles), dim3(RK_THREADS), 0, s, w.key[0], w.key[1], w.val[0], w.val[1], M,
                     w.plan, w.lead_r2, w.trail_r2, rank2);
  hipLaunchKernelGGL(rank_side_stats_kernel, dim3(1), dim3(RK_THREADS), 0, s, w.partial, tiles, M, nan_flag,
                     side_stats);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_spearman_vs_rank2(const float *v, const uint32_t *rank2, const double *side_stats, int64_t M,
                                        double *out, void *ws, size_t ws_bytes, hicgat_stream_t stream) {
  const int rc = rank_check(M, ws, ws_bytes);
  if (rc != HICGAT_OK) return rc;
  if (!v || !rank2 || !side_stats || !out || misaligned(out, 8) || misaligned(side_stats, 8)) return HICGAT_EINVAL;
  const RankWs w = rank_carve(ws, M);
  hipStream_t s = (hipStream_t)stream;
  if (rank_begin(w, s) != HICGAT_OK) return HICGAT_ELAUNCH;
  uint32_t *nan_flag = w.ctrl + 4 * 256;
  hipLaunchKernelGGL(rank_keygen_vec_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, v, M, rank2, w.key[0],
                     w.val[0], nan_flag);
  const int rs = rank_sort_reduce(w, M, s);
  if (rs != HICGAT_OK) return rs;
  hipLaunchKernelGGL(rank_finalize_kernel, dim3(1), dim3(RK_THREADS), 0, s, w.partial, (int)rank_tiles(M), M, nan_flag,
                     side_stats, out);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}

extern "C" int hicgat_dscc_coords(const float *coords, int N, const uint32_t *rank2, const double *side_stats,
                                  double *out, void *ws, size_t ws_bytes, hicgat_stream_t stream) {
  if (N > 65536) return HICGAT_EUNSUPPORTED;
  if (N < 2) return HICGAT_EINVAL;
  const int64_t M = (int64_t)N * (N - 1) / 2;
  const int rc = rank_check(M, ws, ws_bytes);
  if (rc != HICGAT_OK) return rc;
  if (!coords || !rank2 || !side_stats || !out || misaligned(out, 8) || misaligned(side_stats, 8))
    return HICGAT_EINVAL;
  const RankWs w = rank_carve(ws, M);
  hipStream_t s = (hipStream_t)stream;
  if (rank_begin(w, s) != HICGAT_OK) return HICGAT_ELAUNCH;
  uint32_t *nan_flag = w.ctrl + 4 * 256;
  hipLaunchKernelGGL(rank_keygen_coords_kernel, triu_grid(N), dim3(256), 0, s, coords, N, rank2, w.key[0], w.val[0],
                     nan_flag);
  const int rs = rank_sort_reduce(w, M, s);
  if (rs != HICGAT_OK) return rs;
  hipLaunchKernelGGL(rank_finalize_kernel, dim3(1), dim3(RK_THREADS), 0, s, w.partial, (int)rank_tiles(M), M, nan_flag,
                     side_stats, out);
  HICGAT_CHECK_LAUNCH();
  return HICGAT_OK;
}
