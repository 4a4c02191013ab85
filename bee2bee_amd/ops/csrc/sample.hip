// Fused batched sampler: per-row temperature / top-k / top-p / repetition
// penalty and a counter-based RNG keyed by (request seed, output position),
// one workgroup per row of logits [B, V]. Semantics: ops/reference.py
// sample_rows, step for step.
//
// Every element gets a unique 64-bit composite
//     c = (key(z) << nb) | (~index & (2^nb - 1)),   nb = bits of V - 1,
// where key() is the order-preserving u32 image of the fp32 z (NaN -> 0,
// -0 -> +0), so "z descending, index ascending" is plain descending c.
// The k-th largest c is found by radix select, 12 bits per level, with
// integer LDS histograms: one pass over the row per level. As soon as the
// bin that holds the k-th has at most SMP_CAP elements, one more pass
// gathers that bin and everything above it (fewer than k <= 1024 elements)
// into LDS, a bitonic sort orders them, and a scan, the top-p cut and the
// inverse-CDF pick finish the row. Typical rows take two passes; a row of
// all-equal logits takes ceil((32 + nb) / 12) + 1.
//
// Deterministic: the gather order depends on LDS atomics, but the composites
// are unique and sorted before use; sums are a fixed-shape scan. No float
// atomics.
#include "common.h"

#include <stdint.h>

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / WAVE)
#define SMP_MAX_K 1024
#define SMP_DIGIT 12
#define SMP_BINS (1 << SMP_DIGIT)
#define SMP_BUF 4096                       // composites held in LDS
#define SMP_CAP (SMP_BUF - SMP_MAX_K)      // largest bin gathered whole

static_assert(SMP_BINS == 4 * SMP_THREADS, "4 bins per thread in the select");
static_assert(SMP_MAX_K <= SMP_THREADS, "one candidate per thread");

namespace {

DEV_INLINE float smp_to_f(unsigned short v) { return bf2f(v); }
DEV_INLINE float smp_to_f(float v) { return v; }

template <typename T> struct SmpVec;
template <> struct SmpVec<unsigned short> {
    static constexpr int N = 8;
    static DEV_INLINE void load(const unsigned short* p, float* out) {
        load_bf16x8(p, out);
    }
};
template <> struct SmpVec<float> {
    static constexpr int N = 4;
    static DEV_INLINE void load(const float* p, float* out) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    }
};

// f(index, float(logit)) for every element of a row whose base may sit at
// any element offset: scalar head up to the first 16-byte boundary, 16-byte
// vector body, scalar tail.
template <typename T, typename F>
DEV_INLINE void smp_for_each(const T* row, int V, F&& f) {
    constexpr int N = SmpVec<T>::N;
    const int tid = threadIdx.x;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(row);
    BB_KASSERT(addr % sizeof(T) == 0);
    int head = (int)(((16 - (addr & 15)) & 15) / sizeof(T));
    if (head > V) head = V;
    const int nvec = (V - head) / N;
    const int tail0 = head + nvec * N;
    if (tid < head) f(tid, smp_to_f(row[tid]));
    for (int v = tid; v < nvec; v += SMP_THREADS) {
        float e[N];
        SmpVec<T>::load(row + head + v * N, e);
#pragma unroll
        for (int j = 0; j < N; ++j) f(head + v * N + j, e[j]);
    }
    if (tid < V - tail0) f(tail0 + tid, smp_to_f(row[tail0 + tid]));
}

// order-preserving u32 key of z: NaN -> 0 (below -inf), -0 -> +0
DEV_INLINE uint32_t smp_key(float z) {
    if (z == 0.f) z = 0.f;
    const uint32_t b = __float_as_uint(z);
    const uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return (z != z) ? 0u : key;
}

DEV_INLINE float smp_unkey(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// word 0 of Philox4x32-10, counter (pos, 0, 0, 0), key (seed lo, seed hi)
DEV_INLINE uint32_t smp_philox0(uint64_t seed, uint32_t pos) {
    uint32_t c0 = pos, c1 = 0, c2 = 0, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    return c0;
}

// exclusive prefix sum of v over the workgroup's threads
DEV_INLINE int smp_excl_scan(int v, int* wave_tot) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    int incl = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int n = __shfl_up(incl, off);
        if (lane >= off) incl += n;
    }
    if (lane == WAVE - 1) wave_tot[w] = incl;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < w; ++i) base += wave_tot[i];
    __syncthreads();
    return base + incl - v;
}

// inclusive prefix sum, fp32, fixed shape: wave scan, then the wave totals
// added in wave order
DEV_INLINE float smp_incl_scan(float v, float* wave_tot) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    float incl = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const float n = __shfl_up(incl, off);
        if (lane >= off) incl += n;
    }
    if (lane == WAVE - 1) wave_tot[w] = incl;
    __syncthreads();
    float base = 0.f;
    for (int i = 0; i < w; ++i) base += wave_tot[i];
    __syncthreads();
    return base + incl;
}

template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(
    const T* __restrict__ logits, long row_stride, int V,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ penalty,
    const unsigned char* __restrict__ seen_pool, long pool_stride,
    int n_slots, const int* __restrict__ seen_slot,
    const long long* __restrict__ seed, const int* __restrict__ pos,
    long long* __restrict__ out) {
    __shared__ uint64_t buf[SMP_BUF];
    __shared__ unsigned hist[SMP_BINS];   // later: fp32 cum[SMP_MAX_K]
    __shared__ int wave_tot[SMP_WAVES];
    __shared__ float wave_totf[SMP_WAVES];
    __shared__ int sh_bin, sh_need, sh_cnt, sh_count, sh_nkept, sh_first;

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const T* row = logits + (long)b * row_stride;

    const float T_ = fmaxf(temperature[b], 1e-5f);   // NaN -> 1e-5
    const float pen = penalty[b];
    const int kmax = V < SMP_MAX_K ? V : SMP_MAX_K;
    int k = top_k[b];
    k = k < 1 ? 1 : (k > kmax ? kmax : k);
    int slot = seen_pool != nullptr ? seen_slot[b] : -1;
    // values on the device cannot be checked before the launch: a slot past
    // the pool reads as none, like top_k outside 1..kmax is clamped
    if (slot >= n_slots) slot = -1;
    const unsigned char* mrow =
        slot >= 0 ? seen_pool + (long)slot * pool_stride : nullptr;

    const int nb = V > 1 ? 32 - __clz(V - 1) : 0;
    const uint32_t idx_mask = nb ? (0xffffffffu >> (32 - nb)) : 0u;
    const int total_bits = 32 + nb;

    auto composite = [&](int i, float x) -> uint64_t {
        if (mrow != nullptr && mrow[i]) x = x > 0.f ? x / pen : x * pen;
        const float z = __fdiv_rn(x, T_);
        return ((uint64_t)smp_key(z) << nb) | (~(uint32_t)i & idx_mask);
    };

    // ---- radix select of the k-th largest composite
    int hi = total_bits;      // bits [hi, total_bits) are decided: == prefix
    uint64_t prefix = 0;
    int need = k;             // rank wanted among the elements under prefix
    for (;;) {
        const int bits = hi < SMP_DIGIT ? hi : SMP_DIGIT;
        const int lo = hi - bits;
        const unsigned dmask = (1u << bits) - 1u;
        const bool top = hi == total_bits;
#pragma unroll
        for (int j = 0; j < 4; ++j) hist[tid * 4 + j] = 0;
        __syncthreads();
        smp_for_each(row, V, [&](int i, float x) {
            const uint64_t c = composite(i, x);
            if (top || (c >> hi) == prefix)
                atomicAdd(&hist[(unsigned)(c >> lo) & dmask], 1u);
        });
        __syncthreads();
        // thread t owns the bins 4095 - 4t - j, highest first
        unsigned h[4];
        int s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = hist[SMP_BINS - 1 - (tid * 4 + j)];
            s += (int)h[j];
        }
        int above = smp_excl_scan(s, wave_tot);
        if (above < need && above + s >= need) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (above < need && above + (int)h[j] >= need) {
                    sh_bin = SMP_BINS - 1 - (tid * 4 + j);
                    sh_need = need - above;
                    sh_cnt = (int)h[j];
                }
                above += (int)h[j];
            }
        }
        __syncthreads();
        prefix = (prefix << bits) | (uint64_t)sh_bin;
        need = sh_need;
        const int cnt = sh_cnt;
        hi = lo;
        BB_KASSERT(need >= 1 && need <= cnt);
        BB_KASSERT(hi > 0 || cnt == 1);
        __syncthreads();
        if (cnt <= SMP_CAP || hi == 0) break;
    }

    // ---- gather the selected bin and everything above it: count =
    // (k - need) + cnt <= SMP_MAX_K - 1 + SMP_CAP < SMP_BUF
    if (tid == 0) sh_count = 0;
    __syncthreads();
    smp_for_each(row, V, [&](int i, float x) {
        const uint64_t c = composite(i, x);
        if ((c >> hi) >= prefix) {
            const int p = atomicAdd(&sh_count, 1);
            BB_KASSERT(p < SMP_BUF);
            if (p < SMP_BUF) buf[p] = c;
        }
    });
    __syncthreads();
    int count = sh_count;
    BB_KASSERT(count >= k && count <= SMP_BUF);
    if (count > SMP_BUF) count = SMP_BUF;
    int n = 2;
    while (n < count) n <<= 1;
    for (int i = count + tid; i < n; i += SMP_THREADS) buf[i] = 0;
    __syncthreads();

    // ---- bitonic sort, descending
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (n >> 1); i += SMP_THREADS) {
                const int a = 2 * i - (i & (stride - 1));
                const int c = a + stride;
                const uint64_t va = buf[a], vc = buf[c];
                const bool desc = (a & size) == 0;
                if (desc ? va < vc : va > vc) {
                    buf[a] = vc;
                    buf[c] = va;
                }
            }
            __syncthreads();
        }
    }

    // ---- weights, scan, top-p, pick: thread j holds candidate j
    const uint64_t c0 = buf[0];
    const float z0 = smp_unkey((uint32_t)(c0 >> nb));
    if (!(fabsf(z0) <= 3.4028234663852886e38f)) {
        // +inf on top, or no finite entry: the first candidate is the token
        if (tid == 0) {
            const int idx = (int)(~(uint32_t)c0 & idx_mask);
            out[b] = idx < V ? idx : V - 1;
        }
        return;
    }
    float w = 0.f;
    if (tid < k) {
        const float z = smp_unkey((uint32_t)(buf[tid] >> nb));
        if (z == z) w = expf(z - z0);
        if (!(w == w)) w = 0.f;
    }
    float* cum_s = reinterpret_cast<float*>(hist);
    const float cum = smp_incl_scan(w, wave_totf);
    cum_s[tid] = cum;
    if (tid == 0) { sh_nkept = k; sh_first = SMP_MAX_K; }
    __syncthreads();
    const float Z = cum_s[k - 1];
    const float p = top_p[b];
    if (p > 0.f && p < 1.f && tid < k && !(__fdiv_rn(cum - w, Z) <= p))
        atomicMin(&sh_nkept, tid);
    __syncthreads();
    int n_kept = sh_nkept;
    if (n_kept < 1) n_kept = 1;
    const uint32_t r0 = smp_philox0((uint64_t)seed[b], (uint32_t)pos[b]);
    const float u = ((float)(r0 >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float thr = u * cum_s[n_kept - 1];
    if (tid < n_kept && cum > thr) atomicMin(&sh_first, tid);
    __syncthreads();
    if (tid == 0) {
        const int choice = sh_first < n_kept - 1 ? sh_first : n_kept - 1;
        const int idx = (int)(~(uint32_t)buf[choice] & idx_mask);
        BB_KASSERT(idx < V);
        out[b] = idx < V ? idx : V - 1;
    }
}

}  // namespace

extern "C" void launch_sample_rows(
    const void* logits, int is_f32, long row_stride, int B, int V,
    const float* temperature, const int* top_k, const float* top_p,
    const float* penalty, const unsigned char* seen_pool, long pool_stride,
    int n_slots, const int* seen_slot, const long long* seed, const int* pos,
    long long* out, hipStream_t stream) {
    if (is_f32)
        sample_rows_kernel<float><<<B, SMP_THREADS, 0, stream>>>(
            static_cast<const float*>(logits), row_stride, V, temperature,
            top_k, top_p, penalty, seen_pool, pool_stride, n_slots, seen_slot,
            seed, pos, out);
    else
        sample_rows_kernel<unsigned short><<<B, SMP_THREADS, 0, stream>>>(
            static_cast<const unsigned short*>(logits), row_stride, V,
            temperature, top_k, top_p, penalty, seen_pool, pool_stride,
            n_slots, seen_slot, seed, pos, out);
}
