// k_fuse.h -- two ranked lists per query fused into one: Reciprocal Rank Fusion or a convex combination of normalised scores
// (DESIGN.md section 4.8k).
//
// One workgroup of 256 threads per query walks the rule in include/mi355dr.h ("hybrid fusion") literally, everything in LDS:
//   1  both lists are read; an entry without an id, with a NaN value or struck out by its map is dropped, the others are
//      compacted (a block prefix count) -- the compact index c of an entry IS its list (c < n1: list 1) and its rank;
//   2  (mapped id, c) is sorted by (id asc, c asc): a list-2 entry whose predecessor is a list-1 entry with its id is that
//      document's second occurrence -- the two become partners;
//   3  union order: list 1 in list order, then list 2's entries without a partner in list 2's order (a second prefix count);
//   4  convex combination only: column 2 is written out in union order, and ONE lane per column walks its column left to
//      right for min / max / sum (and the squared deviations): the contract fixes the order of those additions, so no tree;
//   5  every document's fused score f, then a sort by (f desc, NaN last, position in union order asc), and the first k_out.
// Plain kernel: no communication between workgroups, no global atomics, every loop bounded by the launch's padded size
// np = next_pow2(w1 + w2) <= kFuseMax.  A (mapped) id that occurs twice in one list makes that query's line unspecified, not
// the accesses: every index is a compact index < m or a slot < w1 + w2 that was validated when it was read.
#pragma once
#include "dev_common.h"

namespace mi355 {

constexpr int kFuseThreads = 256;
constexpr int kFuseWidthMax = 1024;            // entries per list
constexpr int kFuseMax = 2 * kFuseWidthMax;    // the union, and k_out
constexpr int kFusePerThread = kFuseMax / kFuseThreads;
constexpr uint64_t kFusePadKey = 0xFFFFFFFFFFFFFFFFull;  // behind every entry in both sorts ...
constexpr uint64_t kFuseNaNKey = 0xFFFFFFFFFFFFFFFEull;  // ... and a NaN score just in front of it
constexpr unsigned kFusePadPay = 0xFFFFu;

// methods and score modes as include/mi355dr.h numbers them
enum : int { kFuseRrf = 0, kFuseMm = 1, kFuseTmm = 2, kFuseZ = 3, kFuseDbsf = 4 };
enum : int { kFuseOneMinus = 0, kFuseNegate = 1, kFuseAsIs = 2 };

struct FuseStat {  // of one column's present scores
    double lo, hi, mean, sd;
};
struct FuseHead {  // the fixed head of the launch's LDS
    FuseStat st[2];
    int wsum[kFuseThreads / 64];
    int n1;
    int pad[3];
};
constexpr int kFuseHeadBytes = 96;
static_assert(sizeof(FuseHead) == kFuseHeadBytes && kFuseHeadBytes % 16 == 0, "the arrays behind the head stay 16-byte aligned");

// head | key u64[np] | val f64[np] | pay u16[np] | partner i16[np] | c2u i16[np] | slot u16[np]: 24 bytes an entry
__host__ __device__ inline size_t fuse_lds_bytes(int np) { return (size_t)kFuseHeadBytes + (size_t)np * 24; }
static_assert(kFuseHeadBytes + kFuseMax * 24 <= 64 * 1024, "the largest launch stays inside the default 64 KiB of LDS");

struct FuseArgs {
    const double* vals[2];
    const int64_t* ids[2];
    const int64_t* map[2];  // null: identity
    int64_t map_len[2];
    int w[2], mode[2];
    int method;
    int64_t rrf_k;
    double absent;          // 1.0 / (double)(rrf_k + fetch_k + 1)
    double weight, tmin[2];
    int np, k_out;
    double* out_vals;
    int64_t* out_ids;
    int32_t* out_count;
};

// list l's member of a pair of launch arguments (a select, not an indexed copy of the argument block)
template <class T>
__device__ __forceinline__ T fuse_pick(const T (&x)[2], int l) {
    return l ? x[1] : x[0];
}

// exclusive prefix of `v` over the block's threads in thread order, and the block's total; every thread calls it
__device__ __forceinline__ int fuse_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // (the last call's totals have been read)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kFuseThreads / 64; ++w) {
        const int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// ascending (key, pay) over n = a power of two; padding (kFusePadKey, kFusePadPay) is last and equal entries are identical
__device__ __forceinline__ void bitonic_asc_fuse(uint64_t* key, uint16_t* pay, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += kFuseThreads) {
                const int p = i ^ j;
                if (p > i) {
                    const bool asc = ((i & k) == 0);
                    const uint64_t ka = key[i], kb = key[p];
                    const unsigned pa = pay[i], pb = pay[p];
                    const bool b_first = kb < ka || (kb == ka && pb < pa), a_first = ka < kb || (ka == kb && pa < pb);
                    if (asc ? b_first : a_first) {
                        key[i] = kb;
                        key[p] = ka;
                        pay[i] = (uint16_t)pb;
                        pay[p] = (uint16_t)pa;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// f descending as an ascending key: +0.0 and -0.0 are one value, NaN behind every number
__device__ __forceinline__ uint64_t fuse_order_key(double f) {
    if (f != f) return kFuseNaNKey;
    uint64_t b = (uint64_t)__double_as_longlong(f);
    if ((b << 1) == 0) b = 0;
    return ~((b >> 63) ? ~b : (b | 0x8000000000000000ull));
}

// a present score under the column's statistics (include/mi355dr.h, "Normalised score")
__device__ __forceinline__ double fuse_normalise(int method, double s, const FuseStat& st, double tmin) {
    if (method == kFuseMm) {
        const double span = st.hi - st.lo;
        return span == 0.0 ? 0.5 : (s - st.lo) / span;
    }
    if (method == kFuseTmm) {
        const double span = st.hi - tmin;
        return span == 0.0 ? 0.5 : (s - tmin) / span;
    }
    if (method == kFuseZ) return st.sd == 0.0 ? 0.0 : (s - st.mean) / st.sd;
    if (st.sd == 0.0) return 0.5;
    const double lo = st.mean - 3.0 * st.sd, span = (st.mean + 3.0 * st.sd) - lo;
    const double x = (s - lo) / span, y = x < 1.0 ? x : 1.0;
    return y > 0.0 ? y : 0.0;
}

// grid: one workgroup per query; dynamic LDS: fuse_lds_bytes(a.np).  The host has checked the shapes (check_fuse).
__global__ __launch_bounds__(kFuseThreads) void k_fuse_lists(const FuseArgs a) {
    extern __shared__ __align__(16) unsigned char fuse_smem[];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x;
    const int np = a.np, w1 = a.w[0], n = a.w[0] + a.w[1];
    FuseHead* sh = (FuseHead*)fuse_smem;
    uint64_t* key = (uint64_t*)(fuse_smem + kFuseHeadBytes);
    double* val = (double*)(key + np);
    uint16_t* pay = (uint16_t*)(val + np);
    int16_t* partner = (int16_t*)(pay + np);
    int16_t* c2u = partner + np;
    uint16_t* slot = (uint16_t*)(c2u + np);
    double* ov = a.out_vals + q * a.k_out;
    int64_t* oid = a.out_ids + q * a.k_out;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    // thread t owns the E consecutive slots (later: compact indices) from t * E: a count over threads is a count in list order
    const int E = np > kFuseThreads ? np / kFuseThreads : 1, i0 = tid * E;

    // ---- 1: strike out, map, convert, compact
    if (tid == 0) sh->n1 = 0;
    int64_t mid[kFusePerThread];
    double sc[kFusePerThread];
    unsigned ok = 0;
    int cnt = 0, cnt1 = 0;
#pragma unroll
    for (int j = 0; j < kFusePerThread; ++j) {
        const int i = i0 + j;
        mid[j] = -1;
        sc[j] = 0.0;
        if (j < E && i < n) {
            const int l = i >= w1;
            const int64_t at = q * fuse_pick(a.w, l) + (l ? i - w1 : i);
            const int64_t* map = fuse_pick(a.map, l);
            int64_t id = fuse_pick(a.ids, l)[at];
            const double v = fuse_pick(a.vals, l)[at];
            bool has = id >= 0 && v == v;
            if (has && map) {
                has = id < fuse_pick(a.map_len, l);
                if (has) {
                    id = map[id];
                    has = id >= 0;
                }
            }
            if (has) {
                ok |= 1u << j;
                ++cnt;
                cnt1 += !l;
                mid[j] = id;
                const int mode = fuse_pick(a.mode, l);
                sc[j] = mode == kFuseOneMinus ? 1.0 - v : mode == kFuseNegate ? -v : v;
            }
        }
    }
    int m = 0;
    int c = fuse_scan(cnt, sh->wsum, &m);
    if (cnt1) atomicAdd(&sh->n1, cnt1);  // (LDS)
#pragma unroll
    for (int j = 0; j < kFusePerThread; ++j) {
        if (ok >> j & 1u) {
            key[c] = (uint64_t)mid[j];
            val[c] = sc[j];
            pay[c] = (uint16_t)c;
            slot[c] = (uint16_t)(i0 + j);
            ++c;
        }
    }
    const int mp = next_pow2(m);  // (block-uniform, <= np)
    for (int i = tid; i < np; i += kFuseThreads) {
        partner[i] = -1;
        if (i >= m) {
            key[i] = kFusePadKey;
            pay[i] = (uint16_t)kFusePadPay;
        }
    }
    __syncthreads();
    const int n1 = sh->n1;
    if (m == 0) {  // (block-uniform) two empty lists
        for (int t = tid; t < a.k_out; t += kFuseThreads) {
            ov[t] = nan;
            oid[t] = -1;
        }
        if (tid == 0 && a.out_count) a.out_count[q] = 0;
        return;
    }

    // ---- 2: the occurrences of an id side by side, list 1's first; partners
    bitonic_asc_fuse(key, pay, mp);
    for (int p = tid + 1; p < m; p += kFuseThreads) {
        if (key[p] == key[p - 1]) {
            const int cb = pay[p], ca = pay[p - 1];
            if (ca < n1 && cb >= n1) {
                partner[cb] = (int16_t)ca;
                partner[ca] = (int16_t)cb;
            }
        }
    }
    __syncthreads();

    // ---- 3: union order.  c2u[u]: the list-2 entry of the document at position u, -1 without one
    unsigned fresh = 0;
    int cntn = 0;
#pragma unroll
    for (int j = 0; j < kFusePerThread; ++j) {
        const int cc = n1 + i0 + j;
        if (j < E && cc < m && partner[cc] < 0) {
            fresh |= 1u << j;
            ++cntn;
        }
    }
    int n_new = 0;
    int at_new = n1 + fuse_scan(cntn, sh->wsum, &n_new);
#pragma unroll
    for (int j = 0; j < kFusePerThread; ++j)
        if (fresh >> j & 1u) c2u[at_new++] = (int16_t)(n1 + i0 + j);
    for (int u = tid; u < n1; u += kFuseThreads) c2u[u] = partner[u];
    const int U = n1 + n_new;  // <= m
    __syncthreads();

    // ---- 4: column 2 in union order (over `key`: the id sort is done with it), then one lane per column
    if (a.method != kFuseRrf) {
        double* col2 = (double*)key;
        unsigned both = 0;
        int cntp = 0;
#pragma unroll
        for (int j = 0; j < kFusePerThread; ++j) {
            const int u = i0 + j;
            if (j < E && u < n1 && partner[u] >= 0) {
                both |= 1u << j;
                ++cntp;
            }
        }
        int n_both = 0;
        int at2 = fuse_scan(cntp, sh->wsum, &n_both);
#pragma unroll
        for (int j = 0; j < kFusePerThread; ++j)
            if (both >> j & 1u) col2[at2++] = val[partner[i0 + j]];
        for (int u = n1 + tid; u < U; u += kFuseThreads) col2[n_both + (u - n1)] = val[c2u[u]];
        __syncthreads();
        if (tid == 0 || tid == 64) {  // (two waves: the columns run side by side)
            const int l = tid >> 6, cn = l ? n_both + n_new : n1;
            const double* col = l ? col2 : val;
            FuseStat st{0.0, 0.0, 0.0, 0.0};
            if (cn > 0) {
                double sum = 0.0;
                st.lo = st.hi = col[0];
                for (int i = 0; i < cn; ++i) {
                    const double s = col[i];
                    sum = sum + s;
                    if (s < st.lo) st.lo = s;  // (the first of equal values stays: +0.0 / -0.0)
                    if (s > st.hi) st.hi = s;
                }
                st.mean = sum / (double)cn;
                if (a.method == kFuseZ || a.method == kFuseDbsf) {
                    double acc = 0.0;
                    for (int i = 0; i < cn; ++i) {
                        const double d = col[i] - st.mean;
                        acc = acc + d * d;
                    }
                    st.sd = sqrt(acc / (double)cn);
                }
            }
            sh->st[l] = st;
        }
        __syncthreads();
    }

    // ---- 5: scores (registers first: they replace the entries' own in `val`), the order, the first k_out
    const double floor_a = a.method == kFuseZ ? -3.0 : 0.0;
    double f[kFusePerThread];
#pragma unroll
    for (int j = 0; j < kFusePerThread; ++j) {
        const int u = tid + j * kFuseThreads;
        f[j] = 0.0;
        if (u < U) {
            const int c1 = u < n1 ? u : -1, c2 = c2u[u];
            if (a.method == kFuseRrf) {
                double r = 0.0;
                if (c1 >= 0) r = r + 1.0 / (double)(a.rrf_k + c1 + 1);
                if (c2 >= 0) r = r + 1.0 / (double)(a.rrf_k + (c2 - n1) + 1);
                if ((c1 >= 0) != (c2 >= 0)) r = r + a.absent;
                f[j] = r;
            } else {
                const double a1 = c1 >= 0 ? fuse_normalise(a.method, val[c1], sh->st[0], a.tmin[0]) : floor_a;
                const double a2 = c2 >= 0 ? fuse_normalise(a.method, val[c2], sh->st[1], a.tmin[1]) : floor_a;
                f[j] = (a.weight * a1) + ((1.0 - a.weight) * a2);
            }
        }
    }
    __syncthreads();
    const int up = next_pow2(U);
#pragma unroll
    for (int j = 0; j < kFusePerThread; ++j) {
        const int u = tid + j * kFuseThreads;
        if (u < U) {
            val[u] = f[j];
            key[u] = fuse_order_key(f[j]);
            pay[u] = (uint16_t)u;
        } else if (u < up) {
            key[u] = kFusePadKey;
            pay[u] = (uint16_t)kFusePadPay;
        }
    }
    __syncthreads();
    bitonic_asc_fuse(key, pay, up);
    for (int t = tid; t < a.k_out; t += kFuseThreads) {
        double fv = nan;
        int64_t id = -1;
        if (t < U) {
            const int u = pay[t], cc = u < n1 ? u : c2u[u], i = slot[cc], l = i >= w1;
            fv = val[u];
            const int64_t* map = fuse_pick(a.map, l);
            id = fuse_pick(a.ids, l)[q * fuse_pick(a.w, l) + (l ? i - w1 : i)];
            if (map) id = map[id];
        }
        ov[t] = fv;
        oid[t] = id;
    }
    if (tid == 0 && a.out_count) a.out_count[q] = U;
}

}  // namespace mi355
