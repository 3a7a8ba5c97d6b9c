// Weighted k-NN probe on frozen features (Wu et al. 2018, DINO's eval_knn): L2-normalised rows, the exact k nearest bank
// items of every query selected chunk by chunk under a TOTAL order, and the temperature-weighted vote of their labels.
// The similarities themselves are calm_gemm's (queries x a bank chunk, fp32) in a scratch [Nq, n].
//
// The order: similarity descending, then bank index ascending.  Values compare as floats through the order-preserving
// uint32 key of the bits (-0.0 is +0.0, a NaN is -inf); an empty slot (-inf, -1) has key 0, below the key of a real -inf.
// Because the order is total and bank indices are distinct, the state after any chunking of the bank, in any order of the
// chunks, is the same bit for bit.
//
// calm_knn_merge, one workgroup per query row:
//   1. one pass over the row against the state's k-th entry.  Once the state is warm nearly every element fails that one
//      compare (16-byte loads, four keys, one wave vote): the fast path, and a row without a candidate writes nothing.
//      Candidates are appended to LDS through an integer counter; their order there does not matter, they are sorted.
//   2. more candidates than the LDS holds (a cold state): four 8-bit radix-select passes over the candidates' keys, with
//      the histograms in LDS and the row re-read from L2, find the k-th key exactly; an ordered compaction (block scans
//      over consecutive elements) takes every candidate above it and the ties of lowest index, k survivors in all.
//   3. a bitonic sort in LDS of the state and the survivors; the best k go back.
// No float atomics; the integer counters change the order of LDS slots only, never a result.
#include <math.h>

#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int KNN_MAX_K = 256;
constexpr int KNN_MAX_D = 4096;
constexpr int KNN_SORT = 1024;                     // LDS slots of the sort: the state and up to KNN_SORT - k candidates

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// bits of a similarity as stored: a NaN becomes -inf
__device__ __forceinline__ uint32_t knn_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u ? 0xff800000u : u; }
// order-preserving key of stored bits: larger key = larger float, -0.0 == +0.0; the smallest (-inf) is 0x007fffff
__device__ __forceinline__ uint32_t knn_key(uint32_t u) {
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- normalisation ---------------------------------------------------------------------------------------------------------
// One wave per row.  Lane l sums the squares of elements l, l + 64, ... (vector form: of vectors l, l + 64, ...) in
// increasing order, the 64 lane sums meet in the xor butterfly: a fixed order.  VEC: elements per 16-byte load, or 1.
template <class T, int VEC>
__device__ __forceinline__ void load_vec(const T* p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        if constexpr (sizeof(T) == 4) v[0] = p[0];
        else v[0] = bf16_to_f32(p[0]);
    } else if constexpr (sizeof(T) == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = a[i];
    } else {
        const u32x4 a = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(a[i] << 16);
            v[2 * i + 1] = __uint_as_float(a[i] & 0xffff0000u);
        }
    }
}

template <class T, int VEC>
__global__ __launch_bounds__(NT) void knn_normalize_kernel(const T* __restrict__ x, long ld, float* __restrict__ out,
                                                           unsigned long long* __restrict__ bad, long N, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= N) return;                                          // (whole waves: no barrier follows)
    const T* xr = x + row * ld;
    float* o = out + row * (long)D;
    const int nv = D / VEC;
    float ss = 0.f;
    bool finite = true;
    for (int q = lane; q < nv; q += 64) {
        float v[VEC];
        load_vec<T, VEC>(xr + (long)q * VEC, v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            finite = finite && fabsf(v[i]) <= 3.402823466e+38f;
            ss = fmaf(v[i], v[i], ss);
        }
    }
    if (VEC > 1 && lane < D - nv * VEC) {                          // the last D % VEC elements, one lane each
        float v[1];
        load_vec<T, 1>(xr + nv * VEC + lane, v);
        finite = finite && fabsf(v[0]) <= 3.402823466e+38f;
        ss = fmaf(v[0], v[0], ss);
    }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const bool ok = __all(finite) && nrm > 0.f && nrm <= 3.402823466e+38f;
    if (!ok && lane == 0) atomicAdd(bad, 1ull);
    for (int q = lane; q < nv; q += 64) {
        float v[VEC];
        if (ok) load_vec<T, VEC>(xr + (long)q * VEC, v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[(long)q * VEC + i] = ok ? v[i] / nrm : 0.f;
    }
    if (VEC > 1 && lane < D - nv * VEC) {
        float v[1] = {0.f};
        if (ok) load_vec<T, 1>(xr + nv * VEC + lane, v);
        o[nv * VEC + lane] = ok ? v[0] / nrm : 0.f;
    }
}

// ---- selection -----------------------------------------------------------------------------------------------------------
struct KnnRef {                                    // the entry candidates have to beat: the state's k-th
    uint32_t key;
    long idx;
};

__device__ __forceinline__ bool knn_better(uint32_t ka, long ia, uint32_t kb, long ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// f(j, bits) for every element of the row, any order: 16-byte loads between the row's first and last 16-byte boundary
template <class F>
__device__ __forceinline__ void knn_row_each(const float* __restrict__ row, int n, F&& f) {
    const int t = threadIdx.x;
    int head = (int)((4u - ((uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2) & 3u)) & 3u);
    if (head > n) head = n;
    const int nvec = (n - head) >> 2;
    if (t < head) f(t, __float_as_uint(row[t]));
    const u32x4* rv = reinterpret_cast<const u32x4*>(row + head);
    for (int q = t; q < nvec; q += NT) {
        const u32x4 v = rv[q];
        const int j = head + 4 * q;
        f(j, v[0]);
        f(j + 1, v[1]);
        f(j + 2, v[2]);
        f(j + 3, v[3]);
    }
    const int tail0 = head + 4 * nvec;
    if (tail0 + t < n) f(tail0 + t, __float_as_uint(row[tail0 + t]));
}

__global__ __launch_bounds__(NT) void knn_merge_kernel(const float* __restrict__ sims, long ld, long base,
                                                       float* __restrict__ best_sim, long* __restrict__ best_idx, int n, int k) {
    __shared__ uint32_t s_key[KNN_SORT];
    __shared__ uint32_t s_bits[KNN_SORT];
    __shared__ long s_idx[KNN_SORT];
    __shared__ uint32_t hist[NT / 64][256];
    __shared__ int s_cnt, s_digit, s_need;
    __shared__ int s_scan[2][NT / 64];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* row = sims + (long)blockIdx.x * ld;
    float* bs = best_sim + (long)blockIdx.x * k;
    long* bi = best_idx + (long)blockIdx.x * k;
    const int cap = KNN_SORT - k;

    KnnRef ref;                                                    // (every thread reads the same two words)
    ref.idx = bi[k - 1];
    ref.key = ref.idx < 0 ? 0u : knn_key(knn_bits(__float_as_uint(bs[k - 1])));
    if (t == 0) s_cnt = 0;
    __syncthreads();

    // 1. candidates: elements that beat the state's k-th entry
    auto is_cand = [&](int j, uint32_t key) { return key > ref.key || (key == ref.key && base + j < ref.idx); };
    knn_row_each(row, n, [&](int j, uint32_t u) {
        const uint32_t b = knn_bits(u), key = knn_key(b);
        const bool c = is_cand(j, key);
        const unsigned long long m = __ballot(c);                  // of the lanes that are here
        if (m == 0) return;                                        // the fast path once the state is warm
        const int lane_ = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
        int p0 = 0;
        if (lane_ == lead) p0 = atomicAdd(&s_cnt, __popcll(m));    // (an LDS integer counter: slot order only)
        p0 = __shfl(p0, lead, 64);
        if (c) {
            const int p = p0 + __popcll(m & ((1ull << lane_) - 1ull));
            if (p < cap) {
                s_key[k + p] = key;
                s_bits[k + p] = b;
                s_idx[k + p] = base + j;
            }
        }
    });
    __syncthreads();
    int cnt = s_cnt;
    if (cnt == 0) return;                                          // the state stands as it is
    __syncthreads();

    if (cnt > cap) {
        // 2. cold state.  cnt > cap >= k candidates: the k-th largest candidate key, digit by digit from the top
        uint32_t prefix = 0, mask = 0;
        int need = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[0][t] = hist[1][t] = hist[2][t] = hist[3][t] = 0u;
            __syncthreads();
            knn_row_each(row, n, [&](int j, uint32_t u) {
                const uint32_t key = knn_key(knn_bits(u));
                if ((key & mask) == prefix && is_cand(j, key)) atomicAdd(&hist[wave][(key >> shift) & 255u], 1u);
            });
            __syncthreads();
            if (wave == 0) {                                       // bins from 255 down, four per lane; one bin holds the need-th
                uint32_t c[4], s = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int b = 255 - 4 * lane - i;
                    c[i] = hist[0][b] + hist[1][b] + hist[2][b] + hist[3][b];
                    s += c[i];
                }
                uint32_t incl = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += up;
                }
                uint32_t run = incl - s;                           // candidates in higher bins
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (run < (uint32_t)need && run + c[i] >= (uint32_t)need) {
                        s_digit = 255 - 4 * lane - i;
                        s_need = need - (int)run;
                    }
                    run += c[i];
                }
            }
            __syncthreads();
            prefix |= (uint32_t)s_digit << shift;
            mask |= 255u << shift;
            need = s_need;
            __syncthreads();
        }
        // prefix is the k-th key: g = k - need candidates lie above it, and the `need` ties of lowest index come along
        const uint32_t kth = prefix;
        const int g = k - need;
        int run_gt = 0, run_eq = 0;
        for (int j0 = 0; j0 < n; j0 += NT) {                       // consecutive elements: the scan is in index order
            const int j = j0 + t;
            uint32_t b = 0, key = 0;
            bool gt = false, eq = false;
            if (j < n) {
                b = knn_bits(__float_as_uint(row[j]));
                key = knn_key(b);
                if (is_cand(j, key)) {
                    gt = key > kth;
                    eq = key == kth;
                }
            }
            const unsigned long long mg = __ballot(gt), me = __ballot(eq);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (lane == 0) {
                s_scan[0][wave] = __popcll(mg);
                s_scan[1][wave] = __popcll(me);
            }
            __syncthreads();
            int pg = __popcll(mg & below), pe = __popcll(me & below), tg = 0, te = 0;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) {
                if (w < wave) {
                    pg += s_scan[0][w];
                    pe += s_scan[1][w];
                }
                tg += s_scan[0][w];
                te += s_scan[1][w];
            }
            int slot = -1;
            if (gt) slot = k + run_gt + pg;
            else if (eq && run_eq + pe < need) slot = k + g + run_eq + pe;
            if (slot >= 0) {
                s_key[slot] = key;
                s_bits[slot] = b;
                s_idx[slot] = base + j;
            }
            run_gt += tg;
            run_eq += te;
            __syncthreads();
        }
        cnt = k;
    }

    // 3. the state, then the sort of k + cnt entries padded to a power of two with empty slots
    int P = 2;
    while (P < k + cnt) P <<= 1;
    for (int i = t; i < P; i += NT) {
        if (i < k) {
            const long id = bi[i];
            const uint32_t b = knn_bits(__float_as_uint(bs[i]));
            s_idx[i] = id < 0 ? -1 : id;
            s_bits[i] = id < 0 ? 0xff800000u : b;
            s_key[i] = id < 0 ? 0u : knn_key(b);
        } else if (i >= k + cnt) {
            s_idx[i] = -1;
            s_bits[i] = 0xff800000u;
            s_key[i] = 0u;
        }
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < (P >> 1); i += NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool first = (lo & size) == 0;               // this run ends best-first
                const uint32_t kl = s_key[lo], kh = s_key[hi];
                const long il = s_idx[lo], ih = s_idx[hi];
                const bool swap = first ? knn_better(kh, ih, kl, il) : knn_better(kl, il, kh, ih);
                if (swap) {
                    const uint32_t bl = s_bits[lo], bh = s_bits[hi];
                    s_key[lo] = kh; s_key[hi] = kl;
                    s_idx[lo] = ih; s_idx[hi] = il;
                    s_bits[lo] = bh; s_bits[hi] = bl;
                }
            }
            __syncthreads();
        }
    }
    for (int i = t; i < k; i += NT) {
        bs[i] = __uint_as_float(s_bits[i]);
        bi[i] = s_idx[i];
    }
}

// ---- the vote ------------------------------------------------------------------------------------------------------------
// One workgroup per query: the k weights and labels go to LDS, every thread then owns the classes t, t + 256, ... and adds
// the weights of its class in slot order (LDS broadcasts).  k * C compares per query; no atomics.
__global__ __launch_bounds__(NT) void knn_vote_kernel(const float* __restrict__ best_sim, const long* __restrict__ best_idx,
                                                      const long* __restrict__ labels, long Nb, float inv_T,
                                                      float* __restrict__ scores, long ld, int k, int C) {
    __shared__ float w[KNN_MAX_K];
    __shared__ int lab[KNN_MAX_K];
    const int t = threadIdx.x;
    const float* bs = best_sim + (long)blockIdx.x * k;
    const long* bi = best_idx + (long)blockIdx.x * k;
    if (t < k) {
        const long id = bi[t];
        int l = -1;
        float e = 0.f;
        if (id >= 0 && id < Nb) {
            const long y = labels[id];
            if (y >= 0 && y < C) {
                l = (int)y;
                const float s = bs[t], s0 = bs[0];
                e = expf((s == s0 ? 0.f : s - s0) * inv_T);
            }
        }
        w[t] = e;
        lab[t] = l;
    }
    __syncthreads();
    float* out = scores + (long)blockIdx.x * ld;
    for (int c = t; c < C; c += NT) {
        float s = 0.f;
        for (int j = 0; j < k; ++j) s += lab[j] == c ? w[j] : 0.f;
        out[c] = s;
    }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

int calm_knn_normalize(const void* x, int64_t ld, int32_t x_type, float* out, int64_t* bad, int64_t N, int32_t D, void* stream) {
    if (!x || !out || !bad || N < 0 || D < 1 || ld < D) return CALM_E_INVAL;
    if (x_type != CALM_ST_F32 && x_type != CALM_ST_BF16) return CALM_E_INVAL;
    if (D > KNN_MAX_D || N > (int64_t)0x7fffffff * (NT / 64)) return CALM_E_UNSUPP;
    if (!aligned4(out) || (reinterpret_cast<uintptr_t>(x) & (x_type == CALM_ST_F32 ? 3u : 1u))) return CALM_E_LAYOUT;
    if (N == 0) return 0;
    const int grid = (int)((N + NT / 64 - 1) / (NT / 64));
    unsigned long long* b = reinterpret_cast<unsigned long long*>(bad);
    if (x_type == CALM_ST_F32) {
        const float* p = static_cast<const float*>(x);
        if (aligned16(p) && ld % 4 == 0) return calm_launch(knn_normalize_kernel<float, 4>, grid, NT, 0, stream, p, ld, out, b, N, D);
        return calm_launch(knn_normalize_kernel<float, 1>, grid, NT, 0, stream, p, ld, out, b, N, D);
    }
    const uint16_t* p = static_cast<const uint16_t*>(x);
    if (aligned16(p) && ld % 8 == 0) return calm_launch(knn_normalize_kernel<uint16_t, 8>, grid, NT, 0, stream, p, ld, out, b, N, D);
    return calm_launch(knn_normalize_kernel<uint16_t, 1>, grid, NT, 0, stream, p, ld, out, b, N, D);
}

int calm_knn_merge(const float* sims, int64_t ld, int64_t base, float* best_sim, int64_t* best_idx, int64_t Nq, int32_t n,
                   int32_t k, void* stream) {
    if (!sims || !best_sim || !best_idx || k < 1 || n < 1 || Nq < 0 || ld < n || base < 0) return CALM_E_INVAL;
    if (base > INT64_MAX - n) return CALM_E_INVAL;
    if (k > KNN_MAX_K || Nq > 0x7fffffff) return CALM_E_UNSUPP;
    if (!aligned4(sims) || !aligned4(best_sim) || (reinterpret_cast<uintptr_t>(best_idx) & 7u)) return CALM_E_LAYOUT;
    if (Nq == 0) return 0;
    return calm_launch(knn_merge_kernel, (int)Nq, NT, 0, stream, sims, ld, base, best_sim, best_idx, n, k);
}

int calm_knn_vote(const float* best_sim, const int64_t* best_idx, const int64_t* bank_labels, int64_t Nb, float inv_T,
                  float* scores, int64_t ld, int64_t Nq, int32_t k, int32_t C, void* stream) {
    if (!best_sim || !best_idx || !bank_labels || !scores || k < 1 || C < 1 || Nq < 0 || Nb < 0 || ld < C) return CALM_E_INVAL;
    if (!(inv_T > 0.0f) || !(inv_T <= 3.402823466e+38f)) return CALM_E_INVAL;
    if (k > KNN_MAX_K || Nq > 0x7fffffff) return CALM_E_UNSUPP;
    if (!aligned4(best_sim) || !aligned4(scores) || (reinterpret_cast<uintptr_t>(best_idx) & 7u) ||
        (reinterpret_cast<uintptr_t>(bank_labels) & 7u))
        return CALM_E_LAYOUT;
    if (Nq == 0) return 0;
    return calm_launch(knn_vote_kernel, (int)Nq, NT, 0, stream, best_sim, best_idx, bank_labels, Nb, inv_T, scores, ld, k, C);
}

}  // extern "C"
