// Top-N recommendations on the device (qmfx_recommend): for each requested user, the first
// min(N, eligible) eligible items in the order "higher score first, equal scores by ascending
// item index", without the dense n_users × n_items score matrix.
//
//   rec_users_kernel   the requested users' factor rows as doubles, [groups·32][k] in the
//                      [t/8][f][t%8] layout of eval_users_kernel (zero padded);
//   rec_select_kernel  grid (item chunks, groups of 32 users), 4 waves of 8 users: scores a
//                      64-item tile exactly as eval_rank_kernel does (the tile staged through
//                      LDS in 64-column stages, the users' rows wave-uniform through the scalar
//                      cache), then, per user, appends the items that are valid, unseen and
//                      rank before the user's threshold to that user's LDS candidate list
//                      (ballot + prefix count; a list belongs to one wave, so no atomics).
//                      A list that could not take another full tile is pruned by its wave to
//                      the best N in rank order (rank counting in LDS), which also raises the
//                      threshold (the N-th best so far).  Per chunk the ≤ N survivors go to a
//                      global partial buffer [chunk][user][N];
//   rec_merge_kernel   one wave per user: streams the user's chunks × N partial candidates
//                      through the same append / prune steps and writes items (int64), scores
//                      and the count, the unused tail as item −1 / score 0.0.
//
// Scores are eval.hip's: bias (or 0), then one rounded multiply and one rounded add per factor
// in factor order, no fused multiply-add, so they equal the host's double scores bit for bit
// and every user's list is uniquely defined (the chunks hold disjoint items and the order
// compares the global item index, so ties break the same way across chunks).  NaN scores are
// out of contract: the order is not total then (no access leaves a list whatever the scores).
// "Seen" items: the user's ascending list (side-0 CSR row or sorted BPR positives).  A cursor
// per user walks the list with the tiles; the entries inside the tile's item range (the
// window, wave-uniform bounds) are held one per lane and each lane binary-searches them for
// its item with lane shuffles.  Bound: fp64 VALU (2 instructions per multiply-add).
//
// Similar rows (qmfx_similar) are the same selection with the query rows taken from the matrix
// they are ranked against: rec_select_kernel's similarity modes (compile time; the recommend
// instantiation is the kernel it was) rank a side's rows by dot product, or by cosine with the
// row norms of rec_norms_kernel (sqrt of the same unfused sum), and can leave the query's own
// row out by index.  Norms are recomputed per call: O(n·k), about one query's work.
//
// Narrower catalogues: a deny list (qmfx_recommend_without) is one bit per item that
// rec_select_kernel's recommend mode ORs into every user's seen mask, a tile's 64 bits being one
// wave-uniform word; candidate lists (qmfx_recommend_candidates) are cand_select_kernel below,
// which gathers only the listed rows and shares the append / prune / merge steps.
//
// LDS of rec_select_kernel (dynamic, one configuration): 32 lists × 256 × 12 B = 96 KiB, the
// per-user state 1,280 B, the item tile 64 × 66 × sizeof(T): 133,376 B (fp64) / 116,480 B
// (fp32), one workgroup per CU.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace qmfx {
namespace {

constexpr int RC_TI = 64;               // items per tile (one per lane)
constexpr int RC_UW = 8;                // users per wave
constexpr int RC_W = 4;                 // waves per workgroup
constexpr int RC_UG = RC_UW * RC_W;     // users per workgroup
constexpr int RC_KC = 64;               // factor columns per LDS stage
constexpr int RC_KMAX = 256;
constexpr int RC_TS = RC_KC + 2;        // tile row stride (even: 8-byte aligned pairs)
constexpr int RC_CAP = 256;             // candidates per list (≥ kRecMaxN + RC_TI)
constexpr int RC_CHUNK = 512;           // listed candidates per chunk (cand_select_kernel)
static_assert(RC_CHUNK % RC_TI == 0);
static_assert(RC_CAP >= kRecMaxN + RC_TI, "a pruned list must take another full tile");

// dynamic LDS carve (every offset a multiple of 16)
constexpr int RC_OFF_CI = RC_UG * RC_CAP * 8;            // int32 [32][256] items
constexpr int RC_OFF_THR = RC_OFF_CI + RC_UG * RC_CAP * 4;  // double [32] threshold scores
constexpr int RC_OFF_SEEN = RC_OFF_THR + RC_UG * 8;      // uint64 [32] seen mask of the tile
constexpr int RC_OFF_CUR = RC_OFF_SEEN + RC_UG * 8;      // int64 [32] seen-list cursor
constexpr int RC_OFF_END = RC_OFF_CUR + RC_UG * 8;       // int64 [32] seen-list end
constexpr int RC_OFF_THI = RC_OFF_END + RC_UG * 8;       // int32 [32] threshold item (−1: none)
constexpr int RC_OFF_CNT = RC_OFF_THI + RC_UG * 4;       // int32 [32] candidates held
constexpr int RC_OFF_TILE = RC_OFF_CNT + RC_UG * 4;
static_assert(RC_OFF_TILE % 16 == 0);
template <typename T>
constexpr int rec_lds_bytes() {
  return RC_OFF_TILE + RC_TI * RC_TS * (int)sizeof(T);
}
static_assert(rec_lds_bytes<double>() <= 160 * 1024);

#pragma clang fp contract(off)
__device__ __forceinline__ double mul_add_rn(double s, double a, double b) {
  const double p = a * b;
  return s + p;
}
// dot / (na · nb): one rounded multiply, then one correctly rounded divide; 0.0 when the
// product of the norms is not positive (a zero row, or a product that underflows)
__device__ __forceinline__ double cosine_rn(double dot, double na, double nb) {
  const double den = na * nb;
  return den > 0.0 ? dot / den : 0.0;
}
#pragma clang fp contract(on)

// what rec_select_kernel ranks: a user's items by score (qmfx_recommend), or a row's
// neighbours on its own side by dot product or cosine (qmfx_similar); SEL_RECOMMEND_DENY is
// SEL_RECOMMEND with a deny bitmap (a mode of its own, so that the kernel without one stays
// exactly the code it was)
// (plain ints: an unnamed enum in the kernel's signature is mangled differently by the host
// and the device compilation, and the launch then finds no kernel)
constexpr int SEL_RECOMMEND = 0, SEL_SIM_DOT = 1, SEL_SIM_COSINE = 2, SEL_RECOMMEND_DENY = 3;
constexpr bool sel_is_sim(int mode) { return mode == SEL_SIM_DOT || mode == SEL_SIM_COSINE; }
template <typename T, int Mode>
using SelArgs = std::conditional_t<sel_is_sim(Mode), SimArgs<T>, RecArgs<T>>;

// (score a, item a) ranks before (score b, item b)
__device__ __forceinline__ bool rec_before(double sa, int32_t ia, double sb, int32_t ib) {
  return sa > sb || (sa == sb && ia < ib);
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uniform(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffffll));
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// One user's candidate list in LDS (RC_CAP entries), owned by one wave.
struct RecList {
  double* s;
  int32_t* i;
};

// Appends the proposing lanes' (score, item) behind the `cnt` entries held; cnt + 64 ≤ RC_CAP.
__device__ __forceinline__ int rec_append(RecList L, int cnt, bool propose, double s, int32_t item) {
  const uint64_t m = __ballot(propose);
  if (propose) {
    const int slot = cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    L.s[slot] = s;
    L.i[slot] = item;
  }
  return cnt + (int)__popcll(m);
}

// Keeps the best min(cnt, topn) of the cnt ≤ RC_CAP entries, in rank order: every entry counts
// the entries that rank before it (items are distinct, so the ranks are 0..cnt−1) and the
// first topn move to their rank.  Every lane has read the whole list before the first store.
__device__ __forceinline__ int rec_prune(RecList L, int cnt, int topn, int lane) {
  double ms[RC_CAP / 64];
  int32_t mi[RC_CAP / 64];
  int rk[RC_CAP / 64];
#pragma unroll
  for (int r = 0; r < RC_CAP / 64; ++r) {
    const int e = lane + 64 * r;
    ms[r] = e < cnt ? L.s[e] : 0.0;
    mi[r] = e < cnt ? L.i[e] : 0x7fffffff;
    rk[r] = 0;
  }
  for (int j = 0; j < cnt; ++j) {
    const double sj = L.s[j];
    const int32_t ij = L.i[j];
#pragma unroll
    for (int r = 0; r < RC_CAP / 64; ++r) rk[r] += rec_before(sj, ij, ms[r], mi[r]) ? 1 : 0;
  }
#pragma unroll
  for (int r = 0; r < RC_CAP / 64; ++r)
    if (lane + 64 * r < cnt && rk[r] < topn) {
      L.s[rk[r]] = ms[r];
      L.i[rk[r]] = mi[r];
    }
  return cnt < topn ? cnt : topn;
}

// Lanes 0..c−1 hold the ascending window entries v; is `item` among them?  (binary search
// with lane shuffles; c in 1..64, wave-uniform)
__device__ __forceinline__ bool rec_in_window(int32_t v, int c, int32_t item) {
  int pos = 0;  // entries below item
  for (int step = 1 << (31 - __clz(c)); step >= 1; step >>= 1) {
    const int p = pos + step;
    const int32_t vv = __shfl(v, (p - 1) & 63, 64);
    if (p <= c && vv < item) pos = p;
  }
  const int32_t vp = __shfl(v, pos & 63, 64);
  return pos < c && vp == item;
}

template <typename T>
__global__ __launch_bounds__(256) void rec_users_kernel(RecArgs<T> a) {
  // layout [t / 8][f][t % 8] (t relative to the batch's first user): one wave's 8 users at
  // factor f are 64 contiguous bytes
  const int64_t tr = blockIdx.x;
  const int64_t t = a.t_base + tr;
  const T* u = a.U + (t < a.nreq ? a.users[t] * (int64_t)a.kp : 0);
  double* o = a.udbl + (tr / RC_UW) * a.k * RC_UW + (tr % RC_UW);
  for (int f = threadIdx.x; f < a.k; f += blockDim.x)
    o[f * RC_UW] = t < a.nreq ? (double)u[f] : 0.0;
}

// One row's norm per thread: the squares summed in factor order, as mul_add_rn sums a score.
template <typename T>
__global__ __launch_bounds__(256) void rec_norms_kernel(const T* __restrict__ F, int64_t n, int k,
                                                        int kp, double* __restrict__ norms) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const T* row = F + r * kp;
  double s = 0.0;
  // eight loads in flight; kp is a multiple of 16, so they stay inside the row
  for (int f0 = 0; f0 < k; f0 += 8) {
    T v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = row[f0 + j];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (f0 + j < k) s = mul_add_rn(s, (double)v[j], (double)v[j]);
  }
  norms[r] = __builtin_sqrt(s);  // correctly rounded (no fast-math in this build)
}

// Mode SEL_RECOMMEND is qmfx_recommend's kernel, SEL_RECOMMEND_DENY the same with the tile's
// word of the deny bitmap ORed into every user's seen mask.  The similarity modes (a.U == a.I, no bias, no
// seen lists) differ after the dot accumulation only: cosine divides by the two rows' norms,
// and with exclude_self the lane whose row is the query's own row does not propose.
template <typename T, int Mode>
__global__ __launch_bounds__(256) void rec_select_kernel(SelArgs<T, Mode> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* const cand_s = (double*)smem;
  int32_t* const cand_i = (int32_t*)(smem + RC_OFF_CI);
  double* const st_thr = (double*)(smem + RC_OFF_THR);
  unsigned long long* const st_seen = (unsigned long long*)(smem + RC_OFF_SEEN);
  int64_t* const st_cur = (int64_t*)(smem + RC_OFF_CUR);
  int64_t* const st_end = (int64_t*)(smem + RC_OFF_END);
  int32_t* const st_thi = (int32_t*)(smem + RC_OFF_THI);
  int32_t* const st_cnt = (int32_t*)(smem + RC_OFF_CNT);
  T* const tile = (T*)(smem + RC_OFF_TILE);

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t t0 = a.t_base + (int64_t)blockIdx.y * RC_UG;
  const int64_t tw = t0 + w * RC_UW;  // first user of this wave
  const int64_t i0 = (int64_t)blockIdx.x * a.chunk;
  const int64_t i1 = i0 + a.chunk < a.nitems ? i0 + a.chunk : a.nitems;
  // wave-uniform rows, read through the constant address space so they become scalar loads
  typedef const __attribute__((address_space(4))) double* cdptr;
  const cdptr ud = (cdptr)(a.udbl + (tw - a.t_base) * a.k);  // [f][8] for this wave's users
  constexpr bool kSim = sel_is_sim(Mode);

  // The state of this wave's users (only this wave touches it, so no barrier orders it):
  // an empty list without threshold, and the seen-list cursor at the chunk's first item.
  if (lane < RC_UW) {
    const int u = w * RC_UW + lane;
    const int64_t t = tw + lane;
    int64_t lo = 0, end = 0;
    if (!kSim && a.seen_ptr && t < a.nreq) {
      const int64_t row = a.users[t];
      lo = a.seen_ptr[row];
      end = a.seen_ptr[row + 1];
      int64_t hi = end;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)a.seen_col[mid] < i0)
          lo = mid + 1;
        else
          hi = mid;
      }
    }
    st_cur[u] = lo;
    st_end[u] = end;
    st_cnt[u] = 0;
    st_thi[u] = -1;
    st_thr[u] = 0.0;
    st_seen[u] = 0ull;
  }

  for (int64_t ib = i0; ib < i1; ib += RC_TI) {
    const int64_t item = ib + lane;
    const bool valid = item < i1;
    const int32_t item32 = (int32_t)(uint32_t)item;
    double acc[RC_UW];
    const double b0 = (!kSim && a.bias && valid) ? (double)a.bias[item] : 0.0;
#pragma unroll
    for (int g = 0; g < RC_UW; ++g) acc[g] = b0;
    for (int f0 = 0; f0 < a.k; f0 += RC_KC) {
      const int kc = a.k - f0 < RC_KC ? a.k - f0 : RC_KC;
      __syncthreads();
      for (int x = threadIdx.x; x < RC_TI * RC_KC; x += 256) {
        const int r = x / RC_KC, cc = x - r * RC_KC;
        tile[r * RC_TS + cc] = (ib + r < i1 && cc < kc) ? a.I[(ib + r) * a.kp + f0 + cc] : (T)0;
      }
      __syncthreads();
      const T* q = &tile[lane * RC_TS];
      const cdptr u0 = ud + f0 * RC_UW;
      if (kc == RC_KC) {
        // full stage, fully unrolled: every user value is an s_load at an immediate offset
#pragma unroll
        for (int f = 0; f < RC_KC; ++f) {
          const double qf = (double)q[f];
#pragma unroll
          for (int g = 0; g < RC_UW; ++g) acc[g] = mul_add_rn(acc[g], u0[f * RC_UW + g], qf);
        }
      } else {
        for (int f = 0; f < kc; ++f) {
          const double qf = (double)q[f];
#pragma unroll
          for (int g = 0; g < RC_UW; ++g) acc[g] = mul_add_rn(acc[g], u0[f * RC_UW + g], qf);
        }
      }
    }

    // which of the tile's items each user has seen: the list entries below the tile's end
    // (all ≥ ib: the cursor has passed everything below), 64 at a time, one per lane
    if (!kSim && a.seen_ptr) {
      const int64_t iend = ib + RC_TI < i1 ? ib + RC_TI : i1;
      for (int g = 0; g < RC_UW; ++g) {
        const int u = w * RC_UW + g;
        int64_t cur = uniform(st_cur[u]);
        const int64_t end = uniform(st_end[u]);
        bool seen = false;
        for (;;) {
          const int64_t e = cur + lane;
          const int32_t v = e < end ? a.seen_col[e] : 0;
          const int c = (int)__popcll(__ballot(e < end && (int64_t)v < iend));
          if (c == 0) break;
          // every lane searches (no short circuit): the search reads the window through lane
          // shuffles, and a lane that skipped it would not supply its entry to the others
          const bool hit = rec_in_window(v, c, item32);
          seen = seen || hit;
          cur += c;
          if (c < 64) break;
        }
        const unsigned long long m = __ballot(seen);
        if (lane == 0) {
          st_cur[u] = cur;
          st_seen[u] = m;
        }
      }
    }

    // the tile's word of the deny bitmap (tiles start on multiples of 64 items): wave-uniform
    unsigned long long denied = 0ull;
    if constexpr (Mode == SEL_RECOMMEND_DENY) {
      typedef const __attribute__((address_space(4))) unsigned long long* cwptr;
      denied = ((cwptr)a.deny)[ib >> 6];
    }

    // proposals: valid, unseen and not denied (similarity: not the query's own row) and ranking
    // before the user's threshold
    double cn = 0.0;  // this lane's row norm
    if constexpr (Mode == SEL_SIM_COSINE) cn = valid ? a.norms[item] : 0.0;
#pragma unroll
    for (int g = 0; g < RC_UW; ++g) {
      if (tw + g >= a.nreq) break;  // uniform over the wave
      const int u = w * RC_UW + g;
      const int cnt = uniform(st_cnt[u]);
      const int32_t thi = st_thi[u];
      const double ths = st_thr[u];
      int64_t self = -1;  // similarity: the query's own row when that is excluded
      if constexpr (kSim) {
        // the query's row index and norm: wave-uniform, through the constant address space
        typedef const __attribute__((address_space(4))) int64_t* cqptr;
        const int64_t q = ((cqptr)a.users)[tw + g];
        if constexpr (Mode == SEL_SIM_COSINE)  // in place: the proposal below is one text
          acc[g] = cosine_rn(acc[g], ((cdptr)a.norms)[q], cn);
        if (a.exclude_self) self = q;
      }
      const bool seen = kSim ? item == self : (bool)(((st_seen[u] | denied) >> lane) & 1ull);
      const bool propose = valid && !seen && (thi < 0 || rec_before(acc[g], item32, ths, thi));
      const RecList L{cand_s + u * RC_CAP, cand_i + u * RC_CAP};
      const int n = rec_append(L, cnt, propose, acc[g], item32);
      if (lane == 0) st_cnt[u] = n;
    }

    // a list that could not take another full tile, or holds N without a threshold yet, is
    // pruned to the best N; a full list's last entry is the new threshold
    for (int g = 0; g < RC_UW; ++g) {
      const int u = w * RC_UW + g;
      const int cnt = uniform(st_cnt[u]);
      const int thi = uniform(st_thi[u]);
      if (cnt > RC_CAP - RC_TI || (thi < 0 && cnt >= a.topn)) {
        const RecList L{cand_s + u * RC_CAP, cand_i + u * RC_CAP};
        const int n = rec_prune(L, cnt, a.topn, lane);
        if (lane == 0) {
          st_cnt[u] = n;
          if (n == a.topn) {
            st_thr[u] = L.s[n - 1];
            st_thi[u] = L.i[n - 1];
          }
        }
      }
    }
  }

  // the chunk's survivors in rank order → [chunk][user of the batch][topn]
  for (int g = 0; g < RC_UW; ++g) {
    if (tw + g >= a.nreq) break;
    const int u = w * RC_UW + g;
    const RecList L{cand_s + u * RC_CAP, cand_i + u * RC_CAP};
    const int n = rec_prune(L, uniform(st_cnt[u]), a.topn, lane);
    const int64_t slot = (int64_t)blockIdx.x * a.nbatch + (tw + g - a.t_base);
    for (int j = lane; j < n; j += 64) {
      a.part_score[slot * a.topn + j] = L.s[j];
      a.part_item[slot * a.topn + j] = L.i[j];
    }
    if (lane == 0) a.part_cnt[slot] = n;
  }
}

struct RecMergeArgs {
  const double* part_score;
  const int32_t* part_item;
  const int32_t* part_cnt;
  int64_t nchunk, nbatch, t_base, nreq;
  int topn;
  int64_t* items;
  double* scores;
  int32_t* counts;
  // nullptr: user tr's lists are the slots ch · nbatch + tr, ch < nchunk; else the slots
  // woff[t] .. woff[t + 1] (cand_select_kernel's per-user form)
  const int64_t* woff;
};

__global__ __launch_bounds__(64) void rec_merge_kernel(RecMergeArgs a) {
  __shared__ double ls[RC_CAP];
  __shared__ int32_t li[RC_CAP];
  const int lane = threadIdx.x;
  const int64_t tr = blockIdx.x;
  const int64_t t = a.t_base + tr;
  if (t >= a.nreq) return;
  const RecList L{ls, li};
  int cnt = 0;
  int32_t thi = -1;
  double ths = 0.0;
  int64_t nchunk = a.nchunk, slot0 = tr, stride = a.nbatch;
  if (a.woff) {
    slot0 = a.woff[t];
    nchunk = a.woff[t + 1] - slot0;
    stride = 1;
  }
  // the chunks' slots [chunk][topn] as one list, 64 slots at a time
  const int64_t total = nchunk * a.topn;
  for (int64_t e0 = 0; e0 < total; e0 += 64) {
    const int64_t e = e0 + lane;
    bool valid = e < total;
    double s = 0.0;
    int32_t it = 0;
    if (valid) {
      const int64_t ch = e / a.topn;
      const int64_t j = e - ch * a.topn;
      const int64_t slot = slot0 + ch * stride;
      valid = j < a.part_cnt[slot];
      if (valid) {
        s = a.part_score[slot * a.topn + j];
        it = a.part_item[slot * a.topn + j];
      }
    }
    const bool propose = valid && (thi < 0 || rec_before(s, it, ths, thi));
    cnt = uniform(rec_append(L, cnt, propose, s, it));
    if (cnt > RC_CAP - 64 || (thi < 0 && cnt >= a.topn)) {
      cnt = rec_prune(L, cnt, a.topn, lane);
      if (cnt == a.topn) {
        ths = L.s[cnt - 1];
        thi = L.i[cnt - 1];
      }
    }
  }
  cnt = rec_prune(L, cnt, a.topn, lane);
  for (int j = lane; j < a.topn; j += 64) {
    a.items[t * a.topn + j] = j < cnt ? (int64_t)L.i[j] : -1;
    a.scores[t * a.topn + j] = j < cnt ? L.s[j] : 0.0;
  }
  if (lane == 0) a.counts[t] = cnt;
}

template <typename T, int Mode>
hipError_t select(const SelArgs<T, Mode>& a0, hipStream_t s) {
  if (a0.k > RC_KMAX || a0.topn < 1 || a0.topn > kRecMaxN) return hipErrorInvalidValue;
  if (a0.nreq == 0) return hipSuccess;
  SelArgs<T, Mode> a = a0;
  // above 64 KiB of LDS: dynamic shared memory with the function's limit raised
  hipError_t e = hipFuncSetAttribute((const void*)rec_select_kernel<T, Mode>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     rec_lds_bytes<T>());
  if (e != hipSuccess) return e;
  const int64_t groups = (a.nreq + RC_UG - 1) / RC_UG;
  const int64_t nchunk = eval_chunks(a.nreq, a.nitems);
  a.chunk = ((a.nitems + nchunk - 1) / nchunk + RC_TI - 1) / RC_TI * RC_TI;
  // users in batches of eval_batch_groups() groups (grid.y ≤ 65535; the users' fp64 rows and
  // the partial lists are staged per batch)
  const int64_t bg = eval_batch_groups();
  for (int64_t g0 = 0; g0 < groups; g0 += bg) {
    const int64_t ng = groups - g0 < bg ? groups - g0 : bg;
    a.t_base = g0 * RC_UG;
    a.nbatch = ng * RC_UG;
    const int64_t nu = a.nreq - a.t_base < a.nbatch ? a.nreq - a.t_base : a.nbatch;
    hipLaunchKernelGGL(rec_users_kernel<T>, dim3((unsigned)a.nbatch), dim3(256), 0, s,
                       static_cast<const RecArgs<T>&>(a));
    hipLaunchKernelGGL((rec_select_kernel<T, Mode>), dim3((unsigned)nchunk, (unsigned)ng),
                       dim3(256), rec_lds_bytes<T>(), s, a);
    const RecMergeArgs m{a.part_score, a.part_item, a.part_cnt, nchunk, a.nbatch, a.t_base,
                         a.nreq,       a.topn,      a.items,    a.scores, a.counts,
                         nullptr};
    hipLaunchKernelGGL(rec_merge_kernel, dim3((unsigned)nu), dim3(64), 0, s, m);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- candidate lists (qmfx_recommend_candidates) ---------------------------------------------
// The selection of rec_select_kernel over listed items only: rows of I are gathered by index,
// so the work follows the lists' lengths, never the catalogue's.  Lists are cut into chunks of
// RC_CHUNK candidates whose ≤ N survivors go through the partial lists and rec_merge_kernel.
//   Shared list   grid (chunks, groups of 32 users): the dense kernel's shape, 4 waves of 8
//                 users over one tile of 64 gathered rows staged through LDS in 64-column
//                 stages (one wave's load instruction reads 64 columns of one row: 256 / 512
//                 contiguous bytes).
//   Per-user      one wave per work item (user, chunk), 4 independent waves per workgroup and
//                 no barrier: every lane reads its own candidate's row from global memory, 8
//                 values at a time, with the user's row wave-uniform through the scalar cache.
//                 No tile, so 12 KiB of LDS and several workgroups per CU hide the gather.
// Seen items: a lane whose candidate would be proposed binary-searches the user's ascending
// seen list for it (few lanes once the threshold stands).
template <bool Shared>
struct CandShape {
  static constexpr int UW = Shared ? RC_UW : 1;  // users per wave
  static constexpr int NU = UW * RC_W;           // lists per workgroup
  // dynamic LDS carve (every offset a multiple of 16)
  static constexpr int OFF_CI = NU * RC_CAP * 8;            // int32 [NU][256] items
  static constexpr int OFF_THR = OFF_CI + NU * RC_CAP * 4;  // double [NU] threshold scores
  static constexpr int OFF_THI = OFF_THR + NU * 8;          // int32 [NU] threshold item (−1: none)
  static constexpr int OFF_CNT = OFF_THI + NU * 4;          // int32 [NU] candidates held
  static constexpr int OFF_TILE = OFF_CNT + NU * 4;         // shared form: the gathered tile
  static_assert(OFF_TILE % 16 == 0);
  template <typename T>
  static constexpr int lds_bytes() {
    return OFF_TILE + (Shared ? RC_TI * RC_TS * (int)sizeof(T) : 0);
  }
};
static_assert(CandShape<true>::lds_bytes<double>() <= 160 * 1024);

// is `item` in the ascending list col[lo .. end)?
__device__ __forceinline__ bool cand_seen(const int32_t* __restrict__ col, int64_t lo, int64_t end,
                                          int32_t item) {
  int64_t hi = end;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] < item)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < end && col[lo] == item;
}

template <typename T, bool Shared>
__global__ __launch_bounds__(256) void cand_select_kernel(CandArgs<T> a) {
  using S = CandShape<Shared>;
  constexpr int UW = S::UW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* const cand_s = (double*)smem;
  int32_t* const cand_i = (int32_t*)(smem + S::OFF_CI);
  double* const st_thr = (double*)(smem + S::OFF_THR);
  int32_t* const st_thi = (int32_t*)(smem + S::OFF_THI);
  int32_t* const st_cnt = (int32_t*)(smem + S::OFF_CNT);
  [[maybe_unused]] T* const tile = (T*)(smem + S::OFF_TILE);

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // this wave's users tw .. tw + UW (positions in the request), its candidates cand[c0 .. c1)
  // and the partial list of its first user
  int64_t tw, c0, c1, slot0;
  if constexpr (Shared) {
    tw = a.t_base + (int64_t)blockIdx.y * RC_UG + w * RC_UW;
    c0 = (int64_t)blockIdx.x * RC_CHUNK;
    c1 = c0 + RC_CHUNK < a.ncand ? c0 + RC_CHUNK : a.ncand;
    slot0 = (int64_t)blockIdx.x * a.nbatch + (tw - a.t_base);
  } else {
    const int64_t wi = a.w_base + (int64_t)blockIdx.x * RC_W + w;
    if (wi >= a.w_end) return;  // a whole wave; this form has no barrier
    tw = uniform((int64_t)a.wuser[wi]);
    const int64_t b = uniform(a.cptr[tw]), e = uniform(a.cptr[tw + 1]);
    c0 = b + (wi - uniform(a.woff[tw])) * RC_CHUNK;
    c1 = c0 + RC_CHUNK < e ? c0 + RC_CHUNK : e;
    slot0 = wi;
  }
  typedef const __attribute__((address_space(4))) double* cdptr;
  // user tw + g at factor f: ud[f · 8 + g] (rec_users_kernel's layout)
  const int64_t tr = tw - a.t_base;
  const cdptr ud = (cdptr)(a.udbl + (tr / RC_UW) * a.k * RC_UW + (tr % RC_UW));

  if (lane < UW) {
    const int u = w * UW + lane;
    st_cnt[u] = 0;
    st_thi[u] = -1;
    st_thr[u] = 0.0;
  }

  for (int64_t p0 = c0; p0 < c1; p0 += RC_TI) {
    const bool valid = p0 + lane < c1;
    const int32_t item = valid ? a.cand[p0 + lane] : 0;  // row 0 exists: some list is not empty
    double acc[UW];
    const double b0 = (a.bias && valid) ? (double)a.bias[item] : 0.0;
#pragma unroll
    for (int g = 0; g < UW; ++g) acc[g] = b0;
    if constexpr (Shared) {
      for (int f0 = 0; f0 < a.k; f0 += RC_KC) {
        const int kc = a.k - f0 < RC_KC ? a.k - f0 : RC_KC;
        __syncthreads();
        // row r of the tile is lane r's candidate; a wave stages 64 columns of one row at a time
        for (int r = w; r < RC_TI; r += RC_W) {
          const int32_t ri = __shfl(item, r, 64);
          tile[r * RC_TS + lane] =
              (p0 + r < c1 && lane < kc) ? a.I[(int64_t)ri * a.kp + f0 + lane] : (T)0;
        }
        __syncthreads();
        const T* q = &tile[lane * RC_TS];
        const cdptr u0 = ud + f0 * RC_UW;
        if (kc == RC_KC) {
#pragma unroll
          for (int f = 0; f < RC_KC; ++f) {
            const double qf = (double)q[f];
#pragma unroll
            for (int g = 0; g < UW; ++g) acc[g] = mul_add_rn(acc[g], u0[f * RC_UW + g], qf);
          }
        } else {
          for (int f = 0; f < kc; ++f) {
            const double qf = (double)q[f];
#pragma unroll
            for (int g = 0; g < UW; ++g) acc[g] = mul_add_rn(acc[g], u0[f * RC_UW + g], qf);
          }
        }
      }
    } else {
      // eight loads of the lane's own row in flight; kp is a multiple of 16, so they stay
      // inside the row
      const T* row = a.I + (int64_t)item * a.kp;
      for (int f0 = 0; f0 < a.k; f0 += 8) {
        T v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row[f0 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (f0 + j < a.k) acc[0] = mul_add_rn(acc[0], ud[(f0 + j) * RC_UW], (double)v[j]);
      }
    }

    // proposals: listed, ranking before the user's threshold and unseen
#pragma unroll
    for (int g = 0; g < UW; ++g) {
      if (tw + g >= a.nreq) break;  // uniform over the wave
      const int u = w * UW + g;
      const int cnt = uniform(st_cnt[u]);
      const int32_t thi = st_thi[u];
      const double ths = st_thr[u];
      bool propose = valid && (thi < 0 || rec_before(acc[g], item, ths, thi));
      if (a.seen_ptr) {
        const int64_t urow = uniform(a.users[tw + g]);
        const int64_t lo = uniform(a.seen_ptr[urow]), end = uniform(a.seen_ptr[urow + 1]);
        if (propose) propose = !cand_seen(a.seen_col, lo, end, item);
      }
      const RecList L{cand_s + u * RC_CAP, cand_i + u * RC_CAP};
      const int n = rec_append(L, cnt, propose, acc[g], item);
      if (lane == 0) st_cnt[u] = n;
    }

    // as in rec_select_kernel: prune a list that could not take another tile or holds N
    // without a threshold; a full list's last entry is the new threshold
    for (int g = 0; g < UW; ++g) {
      const int u = w * UW + g;
      const int cnt = uniform(st_cnt[u]);
      const int thi = uniform(st_thi[u]);
      if (cnt > RC_CAP - RC_TI || (thi < 0 && cnt >= a.topn)) {
        const RecList L{cand_s + u * RC_CAP, cand_i + u * RC_CAP};
        const int n = rec_prune(L, cnt, a.topn, lane);
        if (lane == 0) {
          st_cnt[u] = n;
          if (n == a.topn) {
            st_thr[u] = L.s[n - 1];
            st_thi[u] = L.i[n - 1];
          }
        }
      }
    }
  }

  // the chunk's survivors in rank order → the partial list of every user
  for (int g = 0; g < UW; ++g) {
    if (tw + g >= a.nreq) break;
    const int u = w * UW + g;
    const RecList L{cand_s + u * RC_CAP, cand_i + u * RC_CAP};
    const int n = rec_prune(L, uniform(st_cnt[u]), a.topn, lane);
    const int64_t slot = slot0 + g;
    for (int j = lane; j < n; j += 64) {
      a.part_score[slot * a.topn + j] = L.s[j];
      a.part_item[slot * a.topn + j] = L.i[j];
    }
    if (lane == 0) a.part_cnt[slot] = n;
  }
}

template <typename T>
hipError_t select_candidates(const CandArgs<T>& a0, hipStream_t s) {
  if (a0.k > RC_KMAX || a0.topn < 1 || a0.topn > kRecMaxN) return hipErrorInvalidValue;
  if (a0.nreq == 0) return hipSuccess;
  CandArgs<T> a = a0;
  hipError_t e = hipFuncSetAttribute((const void*)cand_select_kernel<T, true>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     CandShape<true>::lds_bytes<T>());
  if (e != hipSuccess) return e;
  const bool shared = a.cptr == nullptr;
  const int64_t groups = (a.nreq + RC_UG - 1) / RC_UG;
  const int64_t nchunk = shared ? cand_chunks(a.ncand) : 0;
  // users in batches, as select() takes them
  const int64_t bg = eval_batch_groups();
  for (int64_t g0 = 0; g0 < groups; g0 += bg) {
    const int64_t ng = groups - g0 < bg ? groups - g0 : bg;
    a.t_base = g0 * RC_UG;
    a.nbatch = ng * RC_UG;
    const int64_t nu = a.nreq - a.t_base < a.nbatch ? a.nreq - a.t_base : a.nbatch;
    hipLaunchKernelGGL(rec_users_kernel<T>, dim3((unsigned)a.nbatch), dim3(256), 0, s,
                       static_cast<const RecArgs<T>&>(a));
    if (shared) {
      if (nchunk > 0)
        hipLaunchKernelGGL((cand_select_kernel<T, true>), dim3((unsigned)nchunk, (unsigned)ng),
                           dim3(256), CandShape<true>::lds_bytes<T>(), s, a);
    } else {
      a.w_base = a.h_woff[a.t_base];
      a.w_end = a.h_woff[a.t_base + nu];
      const int64_t nwg = (a.w_end - a.w_base + RC_W - 1) / RC_W;
      if (nwg > 0)
        hipLaunchKernelGGL((cand_select_kernel<T, false>), dim3((unsigned)nwg), dim3(256),
                           CandShape<false>::lds_bytes<T>(), s, a);
    }
    const RecMergeArgs m{a.part_score, a.part_item, a.part_cnt, nchunk,   a.nbatch, a.t_base,
                         a.nreq,       a.topn,      a.items,    a.scores, a.counts,
                         shared ? nullptr : a.woff};
    hipLaunchKernelGGL(rec_merge_kernel, dim3((unsigned)nu), dim3(64), 0, s, m);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename T>
hipError_t similar(const SimArgs<T>& a, hipStream_t s) {
  return a.cosine ? select<T, SEL_SIM_COSINE>(a, s) : select<T, SEL_SIM_DOT>(a, s);
}

template <typename T>
hipError_t factor_norms(const T* F, int64_t n, int k, int kp, double* norms, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rec_norms_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, F, n,
                     k, kp, norms);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_recommend(const RecArgs<float>& a, hipStream_t s) {
  return a.deny ? select<float, SEL_RECOMMEND_DENY>(a, s) : select<float, SEL_RECOMMEND>(a, s);
}
hipError_t launch_recommend(const RecArgs<double>& a, hipStream_t s) {
  return a.deny ? select<double, SEL_RECOMMEND_DENY>(a, s) : select<double, SEL_RECOMMEND>(a, s);
}
int64_t cand_chunks(int64_t n) { return (n + RC_CHUNK - 1) / RC_CHUNK; }
hipError_t launch_recommend_candidates(const CandArgs<float>& a, hipStream_t s) {
  return select_candidates(a, s);
}
hipError_t launch_recommend_candidates(const CandArgs<double>& a, hipStream_t s) {
  return select_candidates(a, s);
}
hipError_t launch_similar(const SimArgs<float>& a, hipStream_t s) { return similar(a, s); }
hipError_t launch_similar(const SimArgs<double>& a, hipStream_t s) { return similar(a, s); }
hipError_t launch_factor_norms(const float* F, int64_t n, int k, int kp, double* norms,
                               hipStream_t s) {
  return factor_norms(F, n, k, kp, norms, s);
}
hipError_t launch_factor_norms(const double* F, int64_t n, int k, int kp, double* norms,
                               hipStream_t s) {
  return factor_norms(F, n, k, kp, norms, s);
}

}  // namespace qmfx
