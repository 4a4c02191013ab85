// Memory-bound fused kernels: RMSNorm, fused add+RMSNorm, RoPE, per-head
// QK-norm + RoPE (Qwen3), SwiGLU, paged-KV store. All bf16 I/O vectorized as short8 (16 B/lane — guide G13:
// hipcc does not auto-vectorize bf16 loads; scalar bf16 is ~2x slower).
//
// These replace what the reference ran inside transformers.generate()
// (bee2bee/hf.py:84-108) — each is one HBM round-trip, fused.
#include "common.h"

// ---------------------------------------------------------------- rmsnorm
// One workgroup per row. Row cached in LDS as fp32 between the two passes
// so the input is read from HBM exactly once.
template <bool FUSED_ADD>
__global__ void rmsnorm_kernel(
    const unsigned short* __restrict__ x,      // [T, H]
    const unsigned short* __restrict__ resid,  // [T, H] or null
    const unsigned short* __restrict__ w,      // [H]
    unsigned short* __restrict__ y,            // [T, H]
    unsigned short* __restrict__ resid_out,    // [T, H] or null
    int H, float eps) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* row = reinterpret_cast<float*>(smem_raw);       // [H]
    __shared__ float red[8];

    const long t = blockIdx.x;
    const unsigned short* xr = x + t * (long)H;
    const unsigned short* rr = FUSED_ADD ? resid + t * (long)H : nullptr;
    unsigned short* ro = FUSED_ADD ? resid_out + t * (long)H : nullptr;

    float sumsq = 0.f;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        float v[8];
        load_bf16x8(xr + i, v);
        if (FUSED_ADD) {
            float r[8];
            load_bf16x8(rr + i, r);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += r[j];
            store_bf16x8(ro + i, v);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            row[i + j] = v[j];
            sumsq += v[j] * v[j];
        }
    }
    // block reduction: wave-level then cross-wave through LDS
    sumsq = wave_sum(sumsq);
    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (lane == 0) red[wid] = sumsq;
    __syncthreads();
    const int nw = blockDim.x / WAVE;
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) total += (i < nw) ? red[i] : 0.f;
    const float inv = rsqrtf(total / (float)H + eps);

    unsigned short* yr = y + t * (long)H;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        float wv[8], o[8];
        load_bf16x8(w + i, wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = row[i + j] * inv * wv[j];
        store_bf16x8(yr + i, o);
    }
}

// -------------------------------------------------------------- layernorm
// GPT-2-family LayerNorm (mean/variance, weight + bias), same one-HBM-read
// structure as rmsnorm_kernel: row cached fp32 in LDS between passes.
template <bool FUSED_ADD>
__global__ void layernorm_kernel(
    const unsigned short* __restrict__ x,      // [T, H]
    const unsigned short* __restrict__ resid,  // [T, H] or null
    const unsigned short* __restrict__ w,      // [H]
    const unsigned short* __restrict__ b,      // [H]
    unsigned short* __restrict__ y,            // [T, H]
    unsigned short* __restrict__ resid_out,    // [T, H] or null
    int H, float eps) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* row = reinterpret_cast<float*>(smem_raw);  // [H]
    __shared__ float red[8], red2[8];

    const long t = blockIdx.x;
    const unsigned short* xr = x + t * (long)H;
    const unsigned short* rr = FUSED_ADD ? resid + t * (long)H : nullptr;
    unsigned short* ro = FUSED_ADD ? resid_out + t * (long)H : nullptr;

    float lsum = 0.f, lsumsq = 0.f;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        float v[8];
        load_bf16x8(xr + i, v);
        if (FUSED_ADD) {
            float r[8];
            load_bf16x8(rr + i, r);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += r[j];
            store_bf16x8(ro + i, v);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            row[i + j] = v[j];
            lsum += v[j];
            lsumsq += v[j] * v[j];
        }
    }
    lsum = wave_sum(lsum);
    lsumsq = wave_sum(lsumsq);
    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (lane == 0) { red[wid] = lsum; red2[wid] = lsumsq; }
    __syncthreads();
    const int nw = blockDim.x / WAVE;
    float tot = 0.f, totsq = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        tot += (i < nw) ? red[i] : 0.f;
        totsq += (i < nw) ? red2[i] : 0.f;
    }
    const float mean = tot / (float)H;
    const float var = totsq / (float)H - mean * mean;
    const float inv = rsqrtf(var + eps);

    unsigned short* yr = y + t * (long)H;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        float wv[8], bv[8], o[8];
        load_bf16x8(w + i, wv);
        load_bf16x8(b + i, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = (row[i + j] - mean) * inv * wv[j] + bv[j];
        store_bf16x8(yr + i, o);
    }
}

// ------------------------------------------------------------------ gelu
// HF gelu_new (tanh approximation) — matches transformers GPT-2 exactly.
__global__ void gelu_kernel(
    const unsigned short* __restrict__ x,  // [N] (flattened, 8-aligned)
    unsigned short* __restrict__ y,
    long n8) {
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < n8;
         idx += (long)gridDim.x * blockDim.x) {
        float v[8], o[8];
        load_bf16x8(x + idx * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float u = v[j];
            const float c = 0.7978845608028654f * (u + 0.044715f * u * u * u);
            o[j] = 0.5f * u * (1.f + tanhf(c));
        }
        store_bf16x8(y + idx * 8, o);
    }
}

// ------------------------------------------------------------------- rope
// Llama rotate-half RoPE, in place on strided q/k views of the fused qkv
// projection. One wave per (token, head); lane owns pair (d, d+hd/2).
// cos/sin tables are host-precomputed fp32 (guide App. B: no device trig).
//
// rope_rotate is the one definition of the rotation, for rope_kernel and
// rope_kv_store_kernel. The two product-and-sums are spelled out as the fma
// each has always compiled to here, so the bits do not depend on what the
// optimizer contracts in a given caller:
//   o1 = fma(x1, c, -(x2 * s)),  o2 = fma(x1, s, x2 * c).
__device__ __forceinline__ void rope_rotate(float x1, float x2, float c,
                                            float s, unsigned short& o1,
                                            unsigned short& o2) {
    o1 = f2bf(__fmaf_rn(x1, c, -__fmul_rn(x2, s)));
    o2 = f2bf(__fmaf_rn(x1, s, __fmul_rn(x2, c)));
}

__global__ void rope_kernel(
    unsigned short* __restrict__ q,  // [T, nq, hd], token stride sq
    unsigned short* __restrict__ k,  // [T, nkv, hd], token stride sk
    const int* __restrict__ pos,     // [T]
    const float* __restrict__ cos_t, // [max_len, hd/2]
    const float* __restrict__ sin_t,
    int T, int nq, int nkv, int hd, long sq, long sk) {
    const int glob_wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int heads = nq + nkv;
    if (glob_wave >= T * heads) return;
    const int t = glob_wave / heads;
    const int h = glob_wave % heads;
    unsigned short* base = (h < nq) ? q + (long)t * sq + (long)h * hd
                                    : k + (long)t * sk + (long)(h - nq) * hd;
    const int half = hd / 2;
    const long tab = (long)pos[t] * half;
    for (int d = lane; d < half; d += WAVE) {
        float c = cos_t[tab + d];
        float s = sin_t[tab + d];
        float x1 = bf2f(base[d]);
        float x2 = bf2f(base[d + half]);
        unsigned short o1, o2;
        rope_rotate(x1, x2, c, s, o1, o2);
        base[d] = o1;
        base[d + half] = o2;
    }
}

// ----------------------------------------------------------- qk_norm_rope
// Qwen3 attention prologue: per-head RMSNorm over head_dim (one [hd] weight
// for all q heads, another for all k heads), then rotate-half RoPE — fused,
// in place on the strided q/k views of the fused qkv projection. Same
// mapping as rope_kernel: one wave per (token, head), lane owns the pairs
// (d, d + hd/2) for d = lane, lane + 64 (hd <= 256). The head lives in
// registers as fp32 between the read and the write; the sum of squares is
// one wave_sum (no LDS, no barrier). Normalise, weight and rotate in fp32;
// the only bf16 rounding is the store. The early exit is wave-uniform
// (glob_wave is), so wave_sum always runs with all 64 lanes: lanes past
// hd/2 add zero to the reduction and store nothing.
#define QKN_PAIRS 2  // pairs per lane: hd/2 <= QKN_PAIRS * WAVE

__global__ void __launch_bounds__(256) qk_norm_rope_kernel(
    unsigned short* __restrict__ q,  // [T, nq, hd], token stride sq
    unsigned short* __restrict__ k,  // [T, nkv, hd], token stride sk
    const int* __restrict__ pos,     // [T]
    const float* __restrict__ cos_t, // [max_len, hd/2]
    const float* __restrict__ sin_t,
    const unsigned short* __restrict__ qw,  // [hd]
    const unsigned short* __restrict__ kw,  // [hd]
    int T, int nq, int nkv, int hd, long sq, long sk, float eps) {
    // wave-uniform by construction; saying so keeps t, h, the base
    // pointers and pos[t] in scalar registers
    const int glob_wave = __builtin_amdgcn_readfirstlane(
        (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE));
    const int lane = threadIdx.x % WAVE;
    const int heads = nq + nkv;
    if (glob_wave >= T * heads) return;
    const int t = glob_wave / heads;
    const int h = glob_wave % heads;
    unsigned short* base = (h < nq) ? q + (long)t * sq + (long)h * hd
                                    : k + (long)t * sk + (long)(h - nq) * hd;
    const unsigned short* w = (h < nq) ? qw : kw;
    const int half = hd / 2;
    BB_KASSERT(half <= QKN_PAIRS * WAVE);
    const long tab = (long)pos[t] * half;

    // Every load is issued before the reduction, so the wave pays one
    // memory latency, not two: tables and weights wait in registers. A lane
    // past hd/2 reads pair 0 (in bounds) and its values are discarded, so
    // the loads are straight-line code; only the stores are predicated.
    float x1[QKN_PAIRS], x2[QKN_PAIRS], c[QKN_PAIRS], s[QKN_PAIRS];
    float w1[QKN_PAIRS], w2[QKN_PAIRS];
#pragma unroll
    for (int i = 0; i < QKN_PAIRS; ++i) {
        if (i * WAVE >= half) break;  // wave-uniform
        const int d = lane + i * WAVE;
        const int dd = d < half ? d : 0;
        x1[i] = bf2f(base[dd]);
        x2[i] = bf2f(base[dd + half]);
        c[i] = cos_t[tab + dd];
        s[i] = sin_t[tab + dd];
        w1[i] = bf2f(w[dd]);
        w2[i] = bf2f(w[dd + half]);
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < QKN_PAIRS; ++i) {
        if (i * WAVE >= half) break;
        const float v = x1[i] * x1[i] + x2[i] * x2[i];
        ss += (lane + i * WAVE < half) ? v : 0.f;
    }
    ss = wave_sum(ss);
    const float inv = rsqrtf(ss / (float)hd + eps);

#pragma unroll
    for (int i = 0; i < QKN_PAIRS; ++i) {
        if (i * WAVE >= half) break;
        const int d = lane + i * WAVE;
        if (d < half) {
            const float n1 = x1[i] * inv * w1[i];
            const float n2 = x2[i] * inv * w2[i];
            base[d] = f2bf(n1 * c[i] - n2 * s[i]);
            base[d + half] = f2bf(n2 * c[i] + n1 * s[i]);
        }
    }
}

// ---------------------------------------------------------- kv_cache_store
// Scatter new K/V rows into the paged pool. One wave per (token, kv head).
__global__ void kv_store_kernel(
    const unsigned short* __restrict__ k,  // [T, nkv, hd], token stride sk
    const unsigned short* __restrict__ v,
    unsigned short* __restrict__ k_cache,  // [nb, nkv, bs, hd]
    unsigned short* __restrict__ v_cache,
    const int* __restrict__ slots,         // [T]
    int T, int nkv, int hd, int bs, long sk, long sv) {
    const int glob_wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (glob_wave >= T * nkv) return;
    const int t = glob_wave / nkv;
    const int h = glob_wave % nkv;
    const int slot = slots[t];
    const int blk = slot / bs, off = slot % bs;
    const long dst = (((long)blk * nkv + h) * bs + off) * hd;
    const unsigned short* ks = k + (long)t * sk + (long)h * hd;
    const unsigned short* vs = v + (long)t * sv + (long)h * hd;
    for (int d = lane * 2; d + 1 < hd; d += WAVE * 2) {
        *reinterpret_cast<short2v*>(k_cache + dst + d) =
            *reinterpret_cast<const short2v*>(ks + d);
        *reinterpret_cast<short2v*>(v_cache + dst + d) =
            *reinterpret_cast<const short2v*>(vs + d);
    }
    if (hd % 2) { /* head dims are even for all supported models */ }
}

// fp8 (OCP e4m3) KV cache variant: quantize at store time (RNE pack), so
// the decode kernels read HALF the bytes. With k_inv/v_inv == nullptr the
// scale is 1.0 (e4m3 covers +-448; post-RMSNorm K/V magnitudes sit well
// inside). With per-kv-head reciprocal scales ([nkv] fp32, both given):
//   byte = e4m3_rne(clamp(x * inv_scale[h], -448, 448))
// The clamp is explicit so the byte never depends on the convert
// instruction's overflow mode; the reciprocal comes from the host, so
// there is no device-side division. h is wave-uniform (one wave per
// (token, head)), so the two scales are scalar loads.
//
// The clamp is a compare and a select per bound, not fminf / fmaxf: those
// return the other operand when one is NaN and would store a NaN input as
// -448 (byte 0xfe), a maximal finite key. Both compares are false for NaN,
// so it reaches the convert and becomes a NaN byte, as in the reference;
// +-inf saturate to +-448. Pinned by
// tests/test_write_path_gpu.py::test_fp8_store_on_every_bf16_pattern[scaled].
__device__ __forceinline__ float clamp_e4m3(float x) {
    x = x > 448.f ? 448.f : x;
    return x < -448.f ? -448.f : x;
}

__global__ void kv_store_fp8_kernel(
    const unsigned short* __restrict__ k,  // [T, nkv, hd] bf16
    const unsigned short* __restrict__ v,
    unsigned char* __restrict__ k_cache,   // [nb, nkv, bs, hd] fp8
    unsigned char* __restrict__ v_cache,
    const int* __restrict__ slots,
    const float* __restrict__ k_inv,       // [nkv] or nullptr (unit scale)
    const float* __restrict__ v_inv,
    int T, int nkv, int hd, int bs, long sk, long sv) {
    const int glob_wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (glob_wave >= T * nkv) return;
    const int t = glob_wave / nkv;
    const int h = glob_wave % nkv;
    const int slot = slots[t];
    const int blk = slot / bs, off = slot % bs;
    const long dst = (((long)blk * nkv + h) * bs + off) * hd;
    const unsigned short* ks = k + (long)t * sk + (long)h * hd;
    const unsigned short* vs = v + (long)t * sv + (long)h * hd;
    if (k_inv != nullptr) {
        const int hu = __builtin_amdgcn_readfirstlane(h);
        const float ki = k_inv[hu], vi = v_inv[hu];
        for (int d = lane * 2; d + 1 < hd; d += WAVE * 2) {
            const short2v kk = *reinterpret_cast<const short2v*>(ks + d);
            const short2v vv = *reinterpret_cast<const short2v*>(vs + d);
            *reinterpret_cast<unsigned short*>(k_cache + dst + d) = f2fp8x2(
                clamp_e4m3(bf2f((unsigned short)kk[0]) * ki),
                clamp_e4m3(bf2f((unsigned short)kk[1]) * ki));
            *reinterpret_cast<unsigned short*>(v_cache + dst + d) = f2fp8x2(
                clamp_e4m3(bf2f((unsigned short)vv[0]) * vi),
                clamp_e4m3(bf2f((unsigned short)vv[1]) * vi));
        }
        return;
    }
    for (int d = lane * 2; d + 1 < hd; d += WAVE * 2) {
        const short2v kk = *reinterpret_cast<const short2v*>(ks + d);
        const short2v vv = *reinterpret_cast<const short2v*>(vs + d);
        *reinterpret_cast<unsigned short*>(k_cache + dst + d) =
            f2fp8x2(bf2f((unsigned short)kk[0]), bf2f((unsigned short)kk[1]));
        *reinterpret_cast<unsigned short*>(v_cache + dst + d) =
            f2fp8x2(bf2f((unsigned short)vv[0]), bf2f((unsigned short)vv[1]));
    }
}

// ------------------------------------------------------------ rope_kv_store
// rope_kernel followed by kv_store_kernel / kv_store_fp8_kernel in one pass:
// q and k are rotated in place, and the rotated k and v go to the paged
// cache. Every q, k and v element is read once, 16 B per lane access.
//
// Work item = one lane = 8 dims [8c, 8c + 8) of a head's first half and the
// matching 8 of its second half, hd / 16 items per head, heads in buffer
// order q, k, v; items are numbered flat over (token, head, c), so no lane
// idles but in the last wave. For a q or k head the item is 8 rotation
// pairs; for a v head it is two 16-byte copies. The lanes of a wave that
// share c and the token read the same cos / sin addresses, so the tables
// cost one pair of 32-byte loads per wave instruction, not one per head.
//
// The cache receives the converter applied to the bf16-ROUNDED rotated
// value, the very bits stored in place, so the result is bit for bit the
// two kernels' (KIND 0: bf16 copy; 1: e4m3; 2: e4m3 of clamp(x * inv[h])).
// Needs hd % 16 == 0, token strides that are multiples of 8 elements and
// 16-byte-aligned bases (the binding checks, and runs the two kernels
// otherwise).
template <int KIND>
__device__ __forceinline__ void kv_row_store8(void* cache, long at, short8 x,
                                              float inv) {
    if (KIND == 0) {
        *reinterpret_cast<short8*>((unsigned short*)cache + at) = x;
        return;
    }
    unsigned short w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float a = bf2f((unsigned short)x[2 * i]);
        float b = bf2f((unsigned short)x[2 * i + 1]);
        if (KIND == 2) {
            a = clamp_e4m3(a * inv);
            b = clamp_e4m3(b * inv);
        }
        w[i] = f2fp8x2(a, b);
    }
    uint2 o;
    o.x = (unsigned int)w[0] | ((unsigned int)w[1] << 16);
    o.y = (unsigned int)w[2] | ((unsigned int)w[3] << 16);
    *reinterpret_cast<uint2*>((unsigned char*)cache + at) = o;
}

template <int KIND>
__global__ void __launch_bounds__(256) rope_kv_store_kernel(
    unsigned short* q,        // [T, nq, hd], token stride sq
    unsigned short* k,        // [T, nkv, hd], token stride sk
    const unsigned short* v,  // [T, nkv, hd], token stride sv
    void* __restrict__ k_cache,  // [nb, nkv, bs, hd] bf16 or fp8
    void* __restrict__ v_cache,
    const int* __restrict__ pos,     // [T]
    const int* __restrict__ slots,   // [T]
    const float* __restrict__ cos_t, // [max_len, hd/2]
    const float* __restrict__ sin_t,
    const float* __restrict__ k_inv, // [nkv], KIND 2 only
    const float* __restrict__ v_inv,
    int T, int nq, int nkv, int hd, int bs, long sq, long sk, long sv) {
    const int lph = hd / 16;  // lanes per head
    const int items = (nq + 2 * nkv) * lph;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)T * items) return;
    const int t = (int)(idx / items);
    const int r = (int)(idx - (long)t * items);
    const int h = r / lph;
    const int d = (r - h * lph) * 8;
    const int half = hd / 2;
    BB_KASSERT(t < T && h < nq + 2 * nkv && d + 8 <= half);

    const bool is_q = h < nq;
    const bool is_v = h >= nq + nkv;
    const int kvh = is_q ? 0 : (is_v ? h - nq - nkv : h - nq);
    const unsigned short* src =
        is_q ? q + (long)t * sq + (long)h * hd
             : (is_v ? v + (long)t * sv + (long)kvh * hd
                     : k + (long)t * sk + (long)kvh * hd);
    short8 x1 = *reinterpret_cast<const short8*>(src + d);
    short8 x2 = *reinterpret_cast<const short8*>(src + d + half);

    if (!is_v) {
        const long tab = (long)pos[t] * half + d;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cos_t + tab);
        const f32x4 c1 = *reinterpret_cast<const f32x4*>(cos_t + tab + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sin_t + tab);
        const f32x4 s1 = *reinterpret_cast<const f32x4*>(sin_t + tab + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float c = j < 4 ? c0[j & 3] : c1[j & 3];
            const float s = j < 4 ? s0[j & 3] : s1[j & 3];
            unsigned short o1, o2;
            rope_rotate(bf2f((unsigned short)x1[j]),
                        bf2f((unsigned short)x2[j]), c, s, o1, o2);
            x1[j] = (short)o1;
            x2[j] = (short)o2;
        }
        unsigned short* dstp = const_cast<unsigned short*>(src);
        *reinterpret_cast<short8*>(dstp + d) = x1;
        *reinterpret_cast<short8*>(dstp + d + half) = x2;
        if (is_q) return;
    }
    const int slot = slots[t];
    const int blk = slot / bs, off = slot % bs;
    const long dst = (((long)blk * nkv + kvh) * bs + off) * hd;
    void* cache = is_v ? v_cache : k_cache;
    const float inv = KIND == 2 ? (is_v ? v_inv[kvh] : k_inv[kvh]) : 1.f;
    kv_row_store8<KIND>(cache, dst + d, x1, inv);
    kv_row_store8<KIND>(cache, dst + d + half, x2, inv);
}

// ----------------------------------------------------------------- swiglu
// out[t, i] = silu(gu[t, i]) * gu[t, I + i]; grid-stride, short8 loads.
__global__ void swiglu_kernel(
    const unsigned short* __restrict__ gu,  // [T, 2I]
    unsigned short* __restrict__ out,       // [T, I]
    long T, long I) {
    const long total = T * I / 8;
    for (long idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        const long t = idx / (I / 8);
        const long i = (idx % (I / 8)) * 8;
        float g[8], u[8], o[8];
        load_bf16x8(gu + t * 2 * I + i, g);
        load_bf16x8(gu + t * 2 * I + I + i, u);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float sig = 1.f / (1.f + __expf(-g[j]));
            o[j] = g[j] * sig * u[j];
        }
        store_bf16x8(out + t * I + i, o);
    }
}

// ------------------------------------------------------------- launchers
extern "C" {

void launch_rmsnorm(const unsigned short* x, const unsigned short* w,
                    unsigned short* y, long T, int H, float eps,
                    hipStream_t stream) {
    const int smem = H * 4;
    hipLaunchKernelGGL((rmsnorm_kernel<false>), dim3(T), dim3(256), smem,
                       stream, x, nullptr, w, y, nullptr, H, eps);
}

void launch_layernorm(const unsigned short* x, const unsigned short* w,
                      const unsigned short* b, unsigned short* y, long T,
                      int H, float eps, hipStream_t stream) {
    const int smem = H * 4;
    hipLaunchKernelGGL((layernorm_kernel<false>), dim3(T), dim3(256), smem,
                       stream, x, nullptr, w, b, y, nullptr, H, eps);
}

void launch_fused_add_layernorm(const unsigned short* x,
                                const unsigned short* resid,
                                const unsigned short* w,
                                const unsigned short* b, unsigned short* y,
                                unsigned short* resid_out, long T, int H,
                                float eps, hipStream_t stream) {
    const int smem = H * 4;
    hipLaunchKernelGGL((layernorm_kernel<true>), dim3(T), dim3(256), smem,
                       stream, x, resid, w, b, y, resid_out, H, eps);
}

void launch_gelu(const unsigned short* x, unsigned short* y, long n,
                 hipStream_t stream) {
    const long n8 = n / 8;
    long blocks = (n8 + 255) / 256;
    if (blocks > 2048) blocks = 2048;  // grid-stride
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(gelu_kernel, dim3(blocks), dim3(256), 0, stream, x, y,
                       n8);
}

void launch_fused_add_rmsnorm(const unsigned short* x,
                              const unsigned short* resid,
                              const unsigned short* w, unsigned short* y,
                              unsigned short* resid_out, long T, int H,
                              float eps, hipStream_t stream) {
    const int smem = H * 4;
    hipLaunchKernelGGL((rmsnorm_kernel<true>), dim3(T), dim3(256), smem,
                       stream, x, resid, w, y, resid_out, H, eps);
}

void launch_rope(unsigned short* q, unsigned short* k, const int* pos,
                 const float* cos_t, const float* sin_t, int T, int nq,
                 int nkv, int hd, long sq, long sk, hipStream_t stream) {
    const long waves = (long)T * (nq + nkv);
    const long blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(rope_kernel, dim3(blocks), dim3(256), 0, stream, q, k,
                       pos, cos_t, sin_t, T, nq, nkv, hd, sq, sk);
}

void launch_qk_norm_rope(unsigned short* q, unsigned short* k, const int* pos,
                         const float* cos_t, const float* sin_t,
                         const unsigned short* qw, const unsigned short* kw,
                         int T, int nq, int nkv, int hd, long sq, long sk,
                         float eps, hipStream_t stream) {
    const long waves = (long)T * (nq + nkv);
    const long blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(qk_norm_rope_kernel, dim3(blocks), dim3(256), 0, stream,
                       q, k, pos, cos_t, sin_t, qw, kw, T, nq, nkv, hd, sq, sk,
                       eps);
}

void launch_kv_store(const unsigned short* k, const unsigned short* v,
                     unsigned short* k_cache, unsigned short* v_cache,
                     const int* slots, int T, int nkv, int hd, int bs,
                     long sk, long sv, hipStream_t stream) {
    const long waves = (long)T * nkv;
    const long blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(kv_store_kernel, dim3(blocks), dim3(256), 0, stream, k,
                       v, k_cache, v_cache, slots, T, nkv, hd, bs, sk, sv);
}

void launch_kv_store_fp8(const unsigned short* k, const unsigned short* v,
                         unsigned char* k_cache, unsigned char* v_cache,
                         const int* slots, const float* k_inv,
                         const float* v_inv, int T, int nkv, int hd, int bs,
                         long sk, long sv, hipStream_t stream) {
    const long waves = (long)T * nkv;
    const long blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(kv_store_fp8_kernel, dim3(blocks), dim3(256), 0,
                       stream, k, v, k_cache, v_cache, slots, k_inv, v_inv, T,
                       nkv, hd, bs, sk, sv);
}

// kind: 0 = bf16 cache, 1 = fp8 cache at unit scale, 2 = fp8 with per-head
// reciprocal scales. The caller has checked hd % 16 == 0, the strides and
// the alignment, and that T * (nq + 2 nkv) * hd / 16 fits an int.
void launch_rope_kv_store(unsigned short* q, unsigned short* k,
                          const unsigned short* v, void* k_cache,
                          void* v_cache, const int* pos, const int* slots,
                          const float* cos_t, const float* sin_t,
                          const float* k_inv, const float* v_inv, int kind,
                          int T, int nq, int nkv, int hd, int bs, long sq,
                          long sk, long sv, hipStream_t stream) {
    const long total = (long)T * (nq + 2 * nkv) * (hd / 16);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define BB_ROPE_KV_STORE(KIND)                                                \
    hipLaunchKernelGGL((rope_kv_store_kernel<KIND>), grid, block, 0, stream,  \
                       q, k, v, k_cache, v_cache, pos, slots, cos_t, sin_t,   \
                       k_inv, v_inv, T, nq, nkv, hd, bs, sq, sk, sv)
    if (kind == 0) BB_ROPE_KV_STORE(0);
    else if (kind == 1) BB_ROPE_KV_STORE(1);
    else BB_ROPE_KV_STORE(2);
#undef BB_ROPE_KV_STORE
}

void launch_swiglu(const unsigned short* gu, unsigned short* out, long T,
                   long I, hipStream_t stream) {
    const long total = T * I / 8;
    long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;  // grid-stride (guide G11)
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(swiglu_kernel, dim3(blocks), dim3(256), 0, stream, gu,
                       out, T, I);
}

}  // extern "C"
