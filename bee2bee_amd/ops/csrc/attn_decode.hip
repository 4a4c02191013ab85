// Paged GQA decode attention — three-stage flash-decoding.
//
// The decode step is memory-bound on KV reads (per key: 2*hd*2 B moved).
// The first single fused kernel (VALU lanes-over-keys scores with q in
// registers, then lanes-over-dims PV) could not reach the HBM roofline: the
// two phases together pushed VGPRs past 100 -> 2 waves/SIMD -> too few
// bytes in flight (measured 1.7-2.5 TB/s vs 6.0 TB/s for each access
// pattern probed in isolation — see probe.hip bw_* kernels). Splitting into
// per-chunk kernels keeps each small, with deep independent-load batches:
//   1. attn_scores:  S = q.K^T + chunk-level softmax -> p, (m,l) scratch
//   2. attn_pv:      partial_o = p.V per chunk (p from scratch, LDS-staged)
//   3. attn_combine: merge chunk partials, normalize, write bf16 out
// Scratch p traffic is ~3% of KV traffic.
//
// How the kernels are put together. Everything a decode kernel does per
// block or per chunk is one __device__ __forceinline__ stage, defined once
// under "shared stages" below:
//   DecBlock            block prologue: b, kvh, L, window edge, first chunk
//   stage_q_mfma        q -> LDS for the MFMA kernels (with the SCALED lift)
//   build_qfrags        B fragments from the staged q
//   mfma_scores_softmax K loads, MFMA, mask, chunk softmax: p in registers,
//                       wave max / sum in `red`
//   chunk_ml            `red` -> the chunk's (m, l)
//   merge_chunk         cross-wave merge, FOLD update or partial write
//   fold_init / fold_epilogue   running state of the FOLD variants
// attn_scores_mfma_kernel and attn_pv_kernel (the split path, hd 64/128)
// and attn_decode_fused_kernel (both in one launch, p kept in LDS) are
// compositions of the same stages, so the fused result is bit for bit the
// split path's by construction: a feature added to a stage reaches both.
// One piece is not a stage: the batched V loop (PV_LOOP) is written out in
// both kernels, for the registers; see the note above attn_pv_kernel.
// The fused kernel holds 4 waves/SIMD with no scratch. launch_attn_decode
// picks between the two paths (attn_decode_plan; measurements in
// docs/KERNELS.md, "Fused scores + PV"). Each kernel's LDS layout has one
// definition (scores_lds / pv_lds / fused_lds) that the kernel carves from
// and the launcher sizes from.
//
// Per-kv-head fp8 scales (scaled fp8 cache, value = float(byte)*scale[h]):
// k_scale multiplies the fp32 SCORE after the dot product / MFMA (never the
// staged q: on the fp8 path q is itself quantized to e4m3, and a typical
// k_scale ~0.05 would push it into subnormals), so the chunk (m, l) come
// from scaled scores and combine / FOLD / out_ml need no change. (The
// scaled MFMA kernel also lifts a staged q that would underflow e4m3 by a
// power of two and divides it back out of the score — see stage_q_mfma.)
// v_scale multiplies the PV accumulator once: where part_o is written
// (non-FOLD) or at the final out write (FOLD). kvh is blockIdx.y, so both
// scales are scalar loads held in an SGPR. The unscaled path: the MFMA
// scores kernel takes a SCALED template flag (a runtime null-pointer branch
// around the multiply made the allocator move the MFMA results through more
// AGPRs and cost the unscaled fp8 instantiations a wave of occupancy; with the flag
// the unscaled code is the same as before); the generic scores kernel and
// the PV kernel use a uniform null-pointer branch, which left their
// register counts unchanged. The bf16 instantiations compile the scale
// code away.
//
// Sliding window (window > 0, Mistral-family): the query at L-1 attends
// keys [lo, L), lo = max(0, L - window). Chunk indices stay absolute, so
// the scratch layout is unchanged; every stage starts its chunk walk at
// c0 = lo / DEC_CHUNK, and in the one chunk that straddles lo a key below
// it is handled exactly like a key >= L: no block-table lookup (the entry
// may point at a page already handed back to the pool), dummy K row, score
// forced to -1e30, p = 0, V row never loaded. WINDOWED is a template flag
// for the reason SCALED is: with it false, lo and c0 fold to 0 and the
// window-off instantiations are the code they were before.
//
// Replaces: the reference's decode path inside transformers.generate()
// (bee2bee/hf.py:84-108). Numerics reference: ops/reference.py attn_decode.
#include <type_traits>

#include "attn_decode.h"
#include "common.h"

#define DEC_BLOCK 256
#define DEC_WAVES 4
static_assert(DEC_CHUNK == DEC_WAVES * WAVE && DEC_CHUNK == DEC_BLOCK,
              "one key per thread, 64 keys per wave");
// LDS pointers carry their address space in the type wherever a shared stage
// takes one. The optimizer simplifies an always-inline function on its own
// before it inlines it, and with plain (flat) pointers it does not yet know
// there that they are LDS; attn_pv_kernel then came out with 5-9 more VGPRs
// at G 5-8 (25 more at G 16) than the same code written in place, and a
// wave less (docs/KERNELS.md, "Shared stages").
#define DEC_LDS __attribute__((address_space(3)))

// Cache policy of the KV stream. A decode step reads every K and V byte
// once, so nothing is gained by keeping them in L2 or the Infinity Cache.
// With a switch at 1 the decode kernels read that stream with non-temporal
// loads (the `nt` bit on global_load). Every K read goes through load_kfrag
// or load_kv_bf16x8 and every V read through load_v_pair, so a switch
// changes the load flavour and nothing else: registers, occupancy and every
// output bit stay what they are at 0. The shipped values follow the
// measurements in docs/KERNELS.md, "Cache policy of the KV stream".
#ifndef DEC_K_NT
#define DEC_K_NT 0
#endif
#ifndef DEC_V_NT
#define DEC_V_NT 1
#endif
template <bool NT, typename T>
__device__ __forceinline__ T dec_ld(const T* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// KV element loaders, templated on the cache storage type:
//   unsigned short = bf16 (2 B/elem), unsigned char = OCP fp8 e4m3 (1 B).
// load_kv_bf16x8: 8 K elements for the generic scores kernel.
template <typename KVT>
__device__ __forceinline__ bf16x8 load_kv_bf16x8(const KVT* p);
template <>
__device__ __forceinline__ bf16x8 load_kv_bf16x8(const unsigned short* p) {
    return dec_ld<DEC_K_NT>(reinterpret_cast<const bf16x8*>(p));
}
template <>
__device__ __forceinline__ bf16x8 load_kv_bf16x8(const unsigned char* p) {
    float f[8];
#if DEC_K_NT
    const uchar8 raw = dec_ld<true>(reinterpret_cast<const uchar8*>(p));
    load_fp8x8(reinterpret_cast<const unsigned char*>(&raw), f);
#else
    load_fp8x8(p, f);
#endif
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (__bf16)f[e];
    return r;
}
// raw 2-element cache pair (batched loads keep the raw bytes in flight,
// converting only when consumed)
template <typename KVT> struct kv_pair_t;
template <> struct kv_pair_t<unsigned short> { short2v v; };
template <> struct kv_pair_t<unsigned char> { u8x2 v; };
// one V pair: the only way the PV loops read the V cache
template <typename KVT>
__device__ __forceinline__ kv_pair_t<KVT> load_v_pair(const KVT* p) {
    kv_pair_t<KVT> r;
    r.v = dec_ld<DEC_V_NT>(reinterpret_cast<const decltype(r.v)*>(p));
    return r;
}
__device__ __forceinline__ float2v kv_pair_f32(kv_pair_t<unsigned short> p) {
    return float2v{bf2f((unsigned short)p.v[0]), bf2f((unsigned short)p.v[1])};
}
__device__ __forceinline__ float2v kv_pair_f32(kv_pair_t<unsigned char> p) {
    unsigned short w = (unsigned short)p.v[0] |
                       ((unsigned short)p.v[1] << 8);
    return fp8x2_2f(w);
}

// MFMA fragment plumbing for the scores stage: bf16 caches feed the bf16
// MFMA; fp8 caches feed v_mfma_f32_16x16x32_fp8_fp8 DIRECTLY (same lane
// map, hardware-verified by test_mfma_fp8_fragment_map) — K bytes go
// straight from the load into the matrix op, no convert VALU. q is
// quantized to e4m3 once at fragment setup (the fp8 cache mode is already
// approximate; documented).
template <typename KVT> struct kfrag_of { using type = bf16x8; };
template <> struct kfrag_of<unsigned char> { using type = long; };
template <typename KVT>
__device__ __forceinline__ typename kfrag_of<KVT>::type load_kfrag(
    const KVT* p) {
    return dec_ld<DEC_K_NT>(
        reinterpret_cast<const typename kfrag_of<KVT>::type*>(p));
}
template <typename KVT>
__device__ __forceinline__ typename kfrag_of<KVT>::type qfrag_from_lds(
    const DEC_LDS unsigned short* p);
template <>
__device__ __forceinline__ bf16x8 qfrag_from_lds<unsigned short>(
    const DEC_LDS unsigned short* p) {
    return *reinterpret_cast<const DEC_LDS bf16x8*>(p);
}
template <>
__device__ __forceinline__ long qfrag_from_lds<unsigned char>(
    const DEC_LDS unsigned short* p) {
    unsigned short w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        w[i] = f2fp8x2(bf2f(p[2 * i]), bf2f(p[2 * i + 1]));
    long r;
    unsigned short* rp = reinterpret_cast<unsigned short*>(&r);
#pragma unroll
    for (int i = 0; i < 4; ++i) rp[i] = w[i];
    return r;
}
__device__ __forceinline__ f32x4 mfma_kq(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_kq(long a, long b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------------ LDS layouts
// One definition per kernel, generic over the address type A: with A =
// char* and the dynamic LDS base the kernel gets its carved pointers, with
// A = int and base 0 the launcher gets the byte count in `end`. Every region
// starts on 8 B (voff holds longs) and q / red on 16 B. The functions are
// force-inlined like the stages: left to the ordinary inliner they cost
// attn_pv_kernel up to 25 VGPRs at G = 16.
#define DEC_LAYOUT __host__ __device__ __forceinline__ constexpr

// both scores kernels: q_s [G][hd] bf16, red [DEC_WAVES][G][2] wave max/sum
template <typename A> struct ScoresLds { A q, red, end; };
template <typename A>
DEC_LAYOUT ScoresLds<A> scores_lds(A base, int G, int hd) {
    ScoresLds<A> l{};
    l.q = base;
    l.red = l.q + ((G * hd * 2 + 15) & ~15);
    l.end = l.red + DEC_WAVES * G * 2 * 4;
    return l;
}
// attn_pv_kernel: p_s [CHUNK][G] f32, voff [CHUNK] long, merge
// [DEC_WAVES][G][hd] f32, then the FOLD running state run [G][hd] f32 and
// runml [G][2] f32
template <typename A> struct PvLds { A p, voff, merge, run, runml, end; };
template <typename A>
DEC_LAYOUT PvLds<A> pv_lds(A base, int G, int hd) {
    PvLds<A> l{};
    l.p = base;
    l.voff = l.p + DEC_CHUNK * G * 4;
    l.merge = l.voff + DEC_CHUNK * 8;
    l.run = l.merge + DEC_WAVES * G * hd * 4;
    l.runml = l.run + G * hd * 4;
    l.end = l.runml + G * 8;
    return l;
}
// attn_decode_fused_kernel: the PV kernel's buffers up to run, then the
// scores kernel's (q_s is dead once a chunk's B fragments are built), then
// runml
template <typename A> struct FusedLds {
    PvLds<A> pv;
    ScoresLds<A> sc;
    A runml, end;
};
template <typename A>
DEC_LAYOUT FusedLds<A> fused_lds(A base, int G, int hd) {
    FusedLds<A> l{};
    l.pv = pv_lds(base, G, hd);
    l.sc = scores_lds(l.pv.runml, G, hd);
    l.runml = l.sc.end;
    l.end = l.runml + G * 8;
    return l;
}
static_assert(fused_lds(0, 16, 128).end == 64128,
              "the fused kernel's largest block must stay under 64 KiB");

// ---------------------------------------------------------- shared stages
// Block prologue: which sequence and kv head, its length, the window's
// lower edge and the first live chunk. With WINDOWED false lo and c0 are
// the constant 0.
template <bool WINDOWED>
struct DecBlock {
    int b, kvh, L, lo, c0;
    __device__ __forceinline__ DecBlock(const int* __restrict__ seq_lens,
                                        int window) {
        b = blockIdx.x;
        kvh = blockIdx.y;
        L = seq_lens[b];
        lo = WINDOWED ? max(0, L - window) : 0;  // first live key
        c0 = WINDOWED ? lo / DEC_CHUNK : 0;      // first live chunk
    }
    // no chunk for this block's blockIdx.z
    __device__ __forceinline__ bool idle() const {
        return (c0 + (int)blockIdx.z) * DEC_CHUNK >= L;
    }
    // a key below the window is treated exactly like a key past L
    __device__ __forceinline__ bool live(int key) const {
        return key < L && (!WINDOWED || key >= lo);
    }
};

// element offset of a key's row in a [nb, nkv, bs, hd] cache
__device__ __forceinline__ long kv_row_off(int page, int nkv, int kvh, int bs,
                                           int key, int hd) {
    return (((long)page * nkv + kvh) * bs + key % bs) * hd;
}

// q staging for the MFMA kernels: q * scale, rounded to bf16, into q_s
// [G][HD]. The caller barriers before it reads q_s.
// SCALED: the fp8 MFMA quantizes the staged q to e4m3 with no scale of
// its own, and a head whose K runs large has a correspondingly small q
// (logits stay O(1)) that would land in e4m3's subnormals or flush to
// zero. So when the block's staged q has amax < 2^-5 (at most one
// binade of it would be normal e4m3) the rows are brought into range by
// a power of two 2^k (exact on bf16: only the exponent moves) taken
// from that amax, amax * 2^k in [128, 256), and 2^-k joins k_scale in
// the one uniform factor applied to the fp32 scores (ksc). At or above 2^-5
// q is staged exactly as on the unscaled path, so there all-ones scales
// reproduce the unscaled output bit for bit. Uses red[0..3].
template <int G, int HD, bool SCALED>
__device__ __forceinline__ void stage_q_mfma(
    const unsigned short* __restrict__ q, long q_stride, float scale, int b,
    int kvh, DEC_LDS unsigned short* q_s, DEC_LDS float* red, float& ksc) {
    const int lane = threadIdx.x % WAVE;
    const int wid = threadIdx.x / WAVE;
    // element i = (g, d) of this kv head's [G][HD] query rows, times scale.
    // (Indexing the rows as one contiguous [G*HD] run reads the same
    // elements but sent the windowed bf16 G16/hd128 fused kernels to scratch.)
    const auto qv = [=](int i) __attribute__((always_inline)) {
        const int g = i / HD, d = i % HD;
        return bf2f(q[(long)b * q_stride + (kvh * G + g) * (long)HD + d]) *
               scale;
    };
    if (SCALED) {
        float amax = 0.f;
        for (int i = threadIdx.x; i < G * HD; i += DEC_BLOCK)
            amax = fmaxf(amax, fabsf(bf2f(f2bf(qv(i)))));
        amax = wave_max(amax);
        if (lane == 0) red[wid] = amax;
        __syncthreads();
        amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const int e = __builtin_amdgcn_readfirstlane(
            (__float_as_int(amax) >> 23) & 0xff);
        float qmul = 1.f;
        if (e >= 8 && e < 122) {  // amax < 2^-5; 2^-k stays a normal float
            qmul = __int_as_float((261 - e) << 23);  // 2^(134 - e)
            ksc *= __int_as_float((e - 7) << 23);    // 2^(e - 134)
        }
        for (int i = threadIdx.x; i < G * HD; i += DEC_BLOCK)
            q_s[i] = f2bf(bf2f(f2bf(qv(i))) * qmul);
    } else {
        for (int i = threadIdx.x; i < G * HD; i += DEC_BLOCK)
            q_s[i] = f2bf(qv(i));
    }
}

// B-fragments from the staged q: col = q head (li), k = dim lg*8+e within
// each kstep
template <int G, int HD, typename KVT>
__device__ __forceinline__ void build_qfrags(
    const DEC_LDS unsigned short* q_s, int lg, int li,
    typename kfrag_of<KVT>::type (&bq)[HD / 32]) {
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
        if (li < G) {
            bq[ks] = qfrag_from_lds<KVT>(q_s + li * HD + ks * 32 + lg * 8);
        } else {
            bq[ks] = typename kfrag_of<KVT>::type{};
        }
    }
}

// One chunk's MFMA scores and chunk softmax (hd 64/128): the G dot products
// per key run on the matrix pipe as S^T tiles = K_tile(16 keys) x q^T(16
// cols, G used). A-fragment rows map exactly to "lane reads its key row's
// 16 B segment", so K streams from HBM straight into MFMA operands — no LDS
// staging, no VALU fma chains, ~70 VGPRs -> high occupancy.
// Fragment maps (verified on HW by tests/test_ops_gpu.py::test_mfma_fragment_map):
//   A (16x32): lane = row (l&15), k = (l>>4)*8+e
//   B (32x16): lane = col (l&15), k = (l>>4)*8+e
//   C (16x16): lane = col (l&15), row = (l>>4)*4+r
// In: bq, and where a key row's page comes from. PAGE_BY_SHUFFLE false: the
// block table `bt`, read by the lane that loads the row. True: `page`, the
// page of key (chunk start + wave*64 + lane) that each lane looked up
// itself, fetched from lane t*16 + li by a wave shuffle. (A callable for
// this cost the windowed bf16 hd-128 fused instantiations 48-84 B/lane of
// scratch at G 4 and G 16; with the flag they have none.) Out: sv, the
// 16 p values of this lane (g = li, keys wave_key0 + t*16 + lg*4 + r at
// sv[t*4 + r]), already rounded to bf16; red[(wid*G + g)*2] = wave max,
// [.. + 1] = wave sum of p. One barrier inside, between the max writes and
// reads; the max and sum slots are distinct words, so none is needed
// between the max reads and the sum writes. The caller barriers before
// anyone reads the sums.
template <int G, int HD, typename KVT, bool SCALED, bool WINDOWED,
          bool PAGE_BY_SHUFFLE>
__device__ __forceinline__ void mfma_scores_softmax(
    const DecBlock<WINDOWED>& blk, const KVT* __restrict__ k_cache, int nkv,
    int bs, float ksc, const typename kfrag_of<KVT>::type (&bq)[HD / 32],
    int wave_key0, int wid, int lg, int li, DEC_LDS float* red,
    const int* bt, int page, float (&sv)[16]) {
    constexpr int KSTEPS = HD / 32;
    constexpr int TILES = WAVE / 16;  // 4 key-tiles of 16 per wave
    using kfrag_t = typename kfrag_of<KVT>::type;

    // all TILES*KSTEPS A-fragments issue before any MFMA (probe-style load
    // batching: 16 independent 16 B loads in flight per wave)
    f32x4 acc[TILES];
    kfrag_t afr[TILES][KSTEPS];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const int key = wave_key0 + t * 16 + li;  // A row = li
        const bool live = blk.live(key);
        const int pg = PAGE_BY_SHUFFLE ? __shfl(page, t * 16 + li)
                                       : (live ? bt[key / bs] : 0);
        // dead keys read a safe dummy row; masked by the score mask below
        // (a key below the window takes the same route: its block-table
        // entry may be stale, so it is never looked up)
        const KVT* kr =
            live ? k_cache + kv_row_off(pg, nkv, blk.kvh, bs, key, HD)
                 : k_cache;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks)
            afr[t][ks] = load_kfrag<KVT>(kr + ks * 32 + lg * 8);
    }
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        f32x4 c{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks)
            c = mfma_kq(afr[t][ks], bq[ks], c);
        acc[t] = c;
    }

    float lmax = -1e30f;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = wave_key0 + t * 16 + lg * 4 + r;
            // SCALED: per-head K dequant scale on the fp32 score
            float v = blk.live(key)
                          ? (SCALED ? acc[t][r] * ksc : acc[t][r])
                          : -1e30f;
            sv[t * 4 + r] = v;
            lmax = fmaxf(lmax, v);
        }
    }
    // reduce over the 4 lane groups holding the same g (stride-16 lanes)
    lmax = fmaxf(lmax, __shfl_xor(lmax, 16));
    lmax = fmaxf(lmax, __shfl_xor(lmax, 32));
    if (lg == 0 && li < G) red[(wid * G + li) * 2] = lmax;
    __syncthreads();
    float M = -1e30f;  // chunk max for this lane's g
    if (li < G) {
#pragma unroll
        for (int w2 = 0; w2 < DEC_WAVES; ++w2)
            M = fmaxf(M, red[(w2 * G + li) * 2]);
    }
    float lsum = 0.f;
#pragma unroll
    for (int i = 0; i < TILES * 4; ++i) {
        // round to bf16 BEFORE summing so l matches the p that PV consumes
        const float pv =
            (sv[i] <= -1e29f) ? 0.f : bf2f(f2bf(__expf(sv[i] - M)));
        sv[i] = pv;
        lsum += pv;
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (lg == 0 && li < G) red[(wid * G + li) * 2 + 1] = lsum;
}

// head g's chunk (m, l) from the wave-level max / sum in `red`
template <int G>
__device__ __forceinline__ void chunk_ml(const DEC_LDS float* red, int g,
                                         float& mc, float& lc) {
    lc = 0.f;
    for (int w2 = 0; w2 < DEC_WAVES; ++w2) lc += red[(w2 * G + g) * 2 + 1];
    mc = -1e30f;
    for (int w2 = 0; w2 < DEC_WAVES; ++w2)
        mc = fmaxf(mc, red[(w2 * G + g) * 2]);
}

// FOLD running state lives in LDS so the hot loop stays at ~64 VGPRs
// (a register version measured 101 VGPRs -> 5 waves/SIMD). Each head
// group g is OWNED by wave g%DEC_WAVES: the per-chunk merge + fold and
// the final normalize run G-way parallel across waves instead of
// serializing on wave 0 (the r1 kernel's measured latency tail), and
// per-g slices stay single-writer so no extra barriers appear.
template <int G>
__device__ __forceinline__ void fold_init(DEC_LDS float* run,
                                          DEC_LDS float* runml, int hd,
                                          int lane, int wid) {
    for (int g = wid; g < G; g += DEC_WAVES) {
        for (int i = lane; i < hd; i += WAVE) run[g * hd + i] = 0.f;
        if (lane == 0) {
            runml[g * 2] = -1e30f;
            runml[g * 2 + 1] = 0.f;
        }
    }
}

// Cross-wave merge of one chunk's PV partials (all waves used the same
// chunk max, so it is a plain sum), then per owned head g either the FOLD
// online update of (run, runml) with the chunk's (m, l), or the partial
// write of part_o scaled by vsc. Where the chunk's (m, l) come from:
// ML_FROM_RED false (split path): ml_in, the part_ml the scores kernel
// wrote, read iff FOLD. True (fused): `red`, reduced here by chunk_ml, and
// without FOLD also written to ml_out, the part_ml for combine.
// base = ((b*nkv + kvh)*C + chunk)*G. One barrier inside; the caller
// barriers before the LDS buffers are reused.
template <int G, bool FOLD, bool ML_FROM_RED>
__device__ __forceinline__ void merge_chunk(
    const float (&o0)[G], const float (&o1)[G], int hd, int lane, int wid,
    DEC_LDS float* merge, DEC_LDS float* run, DEC_LDS float* runml,
    float* __restrict__ part_o, float* __restrict__ ml_out,
    const float* __restrict__ ml_in, const DEC_LDS float* red, long base,
    bool scaled, float vsc) {
    const int d0 = lane * 2;
    DEC_LDS float* mw = merge + wid * G * hd;
    if (d0 < hd) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            mw[g * hd + d0] = o0[g];
            mw[g * hd + d0 + 1] = o1[g];
        }
    }
    __syncthreads();
    if (d0 < hd) {
        for (int g = wid; g < G; g += DEC_WAVES) {
            float a0 = 0.f, a1 = 0.f;
            for (int w2 = 0; w2 < DEC_WAVES; ++w2) {
                a0 += merge[(w2 * G + g) * hd + d0];
                a1 += merge[(w2 * G + g) * hd + d0 + 1];
            }
            float mc = 0.f, lc = 0.f;
            if (ML_FROM_RED) {
                chunk_ml<G>(red, g, mc, lc);
            } else if (FOLD) {
                mc = ml_in[(base + g) * 2];
                lc = ml_in[(base + g) * 2 + 1];
            }
            if (FOLD) {
                const float mold = runml[g * 2];
                const float mn = fmaxf(mold, mc);
                const float alpha = __expf(mold - mn);
                const float beta = __expf(mc - mn);
                run[g * hd + d0] = run[g * hd + d0] * alpha + a0 * beta;
                run[g * hd + d0 + 1] =
                    run[g * hd + d0 + 1] * alpha + a1 * beta;
                if (lane == 0) {
                    runml[g * 2] = mn;
                    runml[g * 2 + 1] = runml[g * 2 + 1] * alpha + lc * beta;
                }
            } else {
                if (scaled) {  // per-head V dequant scale, once
                    a0 *= vsc;
                    a1 *= vsc;
                }
                float* po = part_o + (base + g) * hd;
                po[d0] = a0;
                po[d0 + 1] = a1;
                if (ML_FROM_RED && lane == 0) {
                    ml_out[(base + g) * 2] = mc;
                    ml_out[(base + g) * 2 + 1] = lc;
                }
            }
        }
    }
}

// FOLD epilogue: normalize the running state and write the bf16 out rows
// and, where asked for, the final (m, l) per q head
template <int G>
__device__ __forceinline__ void fold_epilogue(
    const DEC_LDS float* run, const DEC_LDS float* runml,
    unsigned short* __restrict__ out,
    float* __restrict__ out_ml, int b, int kvh, int nkv, int hd, int lane,
    int wid, bool scaled, float vsc) {
    const int d0 = lane * 2;
    const int nq = nkv * G;
    if (d0 < hd) {
        for (int g = wid; g < G; g += DEC_WAVES) {
            const float lr = runml[g * 2 + 1];
            const float inv = (lr > 0.f) ? 1.f / lr : 0.f;
            unsigned short* orow = out + ((long)b * nq + kvh * G + g) * hd;
            float r0 = run[g * hd + d0] * inv;
            float r1 = run[g * hd + d0 + 1] * inv;
            if (scaled) {  // per-head V dequant scale, once
                r0 *= vsc;
                r1 *= vsc;
            }
            orow[d0] = f2bf(r0);
            orow[d0 + 1] = f2bf(r1);
        }
    }
    if (out_ml != nullptr && lane == 0) {
        for (int g = wid; g < G; g += DEC_WAVES) {
            float* mlrow = out_ml + ((long)b * nq + kvh * G + g) * 2;
            mlrow[0] = runml[g * 2];
            mlrow[1] = runml[g * 2 + 1];
        }
    }
}

// ------------------------------------------------------------ stage 1: S
// Generic scores kernel for the tail-model head sizes (hd 16/24/96/...):
// one key per thread, VALU dot products against the LDS-held q. hd 64 and
// 128 never come here: launch_attn_decode sends them to the MFMA kernel.
// The key row is read in batches of DEC_KBATCH independent 16 B loads that
// all issue before the first fma: a lane reads its own row, so the loads of
// one lane are the only ones it can overlap. (A loop of one load per step
// measured 1277 us against 807 for scores + PV at hd 96 / G4 / B768, at
// seven times the occupancy; docs/KERNELS.md, "Shared stages".)
#define DEC_KBATCH 8
template <int G, typename KVT, bool WINDOWED>
__global__ __launch_bounds__(DEC_BLOCK) void attn_scores_kernel(
    const unsigned short* __restrict__ q,        // [B, nq, hd] (strided)
    const KVT* __restrict__ k_cache,             // [nb, nkv, bs, hd]
    const int* __restrict__ block_table,         // [B, W]
    const int* __restrict__ seq_lens,            // [B]
    unsigned short* __restrict__ p_out,          // [B, nkv, C, CHUNK, G] bf16
    float* __restrict__ part_ml,                 // [B, nkv, C, G, 2]
    int nkv, int W, int bs, int hd, int C, long q_stride, float scale,
    const float* __restrict__ k_scale,           // [nkv] or nullptr
    int window) {                                // read iff WINDOWED
    const DecBlock<WINDOWED> blk(seq_lens, window);
    if (blk.idle()) return;
    const int b = blk.b, kvh = blk.kvh, L = blk.L;
    const int lane = threadIdx.x % WAVE;
    const int wid = threadIdx.x / WAVE;
    const bool scaled = sizeof(KVT) == 1 && k_scale != nullptr;
    const float ksc = scaled ? k_scale[kvh] : 1.f;

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const auto lds = scores_lds(0, G, hd);
    unsigned short* q_s = reinterpret_cast<unsigned short*>(smem_raw + lds.q);
    float* red = reinterpret_cast<float*>(smem_raw + lds.red);

    for (int i = threadIdx.x; i < G * hd; i += DEC_BLOCK) {
        const int g = i / hd, d = i % hd;
        q_s[i] = f2bf(
            bf2f(q[(long)b * q_stride + (kvh * G + g) * (long)hd + d]) * scale);
    }
    __syncthreads();

    const int* bt = block_table + (long)b * W;
    // loop chunks with stride gridDim.z — the PV and combine stages walk
    // ALL chunks of (b, kvh), so every chunk's p/(m,l) must be produced even
    // when the launcher picks Z < ceil(L/DEC_CHUNK) (a single-
    // chunk kernel left chunks >= Z uninitialized for hd not in {64,128})
    for (int chunk = blk.c0 + blockIdx.z; chunk * DEC_CHUNK < L;
         chunk += gridDim.z) {
    const int start = chunk * DEC_CHUNK;
    const int key = start + threadIdx.x;  // one key per thread
    const bool valid = blk.live(key);

    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = -1e30f;
    if (valid) {
        const int page = bt[key / bs];
        BB_KASSERT(page >= 0);  // block table row must be fully mapped
        const KVT* kr = k_cache + kv_row_off(page, nkv, kvh, bs, key, hd);
#pragma unroll
        for (int g = 0; g < G; ++g) s[g] = 0.f;
        for (int d0 = 0; d0 < hd; d0 += 8 * DEC_KBATCH) {
            bf16x8 kraw[DEC_KBATCH];
#pragma unroll
            for (int u = 0; u < DEC_KBATCH; ++u)
                if (d0 + u * 8 < hd)  // uniform
                    kraw[u] = load_kv_bf16x8<KVT>(kr + d0 + u * 8);
#pragma unroll
            for (int u = 0; u < DEC_KBATCH; ++u) {
                const int d = d0 + u * 8;
                if (d < hd) {
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const short8 qraw =
                            *reinterpret_cast<const short8*>(q_s + g * hd + d);
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            s[g] = fmaf((float)kraw[u][j],
                                        bf2f((unsigned short)qraw[j]), s[g]);
                    }
                }
            }
        }
        if (scaled) {
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] *= ksc;
        }
    }

    // chunk-level softmax: wave max -> LDS -> chunk max; then exp + sums
    float wmax[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wmax[g] = wave_max(s[g]);
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) red[(wid * G + g) * 2] = wmax[g];
    }
    __syncthreads();
    float M[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float m = red[g * 2];
        for (int w2 = 1; w2 < DEC_WAVES; ++w2)
            m = fmaxf(m, red[(w2 * G + g) * 2]);
        M[g] = m;
    }
    float p[G], wsum[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        // round to bf16 BEFORE summing so l matches the p that PV consumes
        p[g] = valid ? bf2f(f2bf(__expf(s[g] - M[g]))) : 0.f;
        wsum[g] = wave_sum(p[g]);
    }
    __syncthreads();  // red reuse (second slot written below)
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) red[(wid * G + g) * 2 + 1] = wsum[g];
    }
    // coalesced p write: [key][G] bf16 (p in [0,1]; bf16 halves the
    // G-proportional scratch traffic)
    {
        unsigned short* prow =
            p_out + ((((long)b * nkv + kvh) * C + chunk) * DEC_CHUNK +
                     threadIdx.x) * G;
#pragma unroll
        for (int g = 0; g < G; ++g) prow[g] = f2bf(p[g]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* pml = part_ml + ((((long)b * nkv + kvh) * C + chunk) * G) * 2;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float lsum = 0.f;
            for (int w2 = 0; w2 < DEC_WAVES; ++w2)
                lsum += red[(w2 * G + g) * 2 + 1];
            pml[g * 2] = M[g];
            pml[g * 2 + 1] = lsum;
        }
    }
    __syncthreads();  // red reused by the next chunk iteration
    }  // chunk loop
}

// MFMA variant of stage 1 (hd 64/128): stage_q_mfma once, then per chunk
// mfma_scores_softmax with each key row's page read from the block table,
// p written to the bf16 scratch and (m, l) to part_ml.
template <int G, int HD, typename KVT, bool SCALED, bool WINDOWED>
__global__ __launch_bounds__(DEC_BLOCK) void attn_scores_mfma_kernel(
    const unsigned short* __restrict__ q,
    const KVT* __restrict__ k_cache,
    const int* __restrict__ block_table,
    const int* __restrict__ seq_lens,
    unsigned short* __restrict__ p_out,  // bf16
    float* __restrict__ part_ml,
    int nkv, int W, int bs, int C, long q_stride, float scale,
    const float* __restrict__ k_scale,    // [nkv]; read iff SCALED
    int window) {                         // read iff WINDOWED
    constexpr int TILES = WAVE / 16;
    const DecBlock<WINDOWED> blk(seq_lens, window);
    if (blk.idle()) return;
    const int b = blk.b, kvh = blk.kvh, L = blk.L;
    float ksc = 1.f;
    if (SCALED) ksc = k_scale[kvh];  // uniform: one scalar load
    const int lane = threadIdx.x % WAVE;
    const int wid = threadIdx.x / WAVE;
    const int lg = lane >> 4;  // lane group 0..3
    const int li = lane & 15;

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const auto lds = scores_lds((DEC_LDS char*)smem_raw, G, HD);
    DEC_LDS unsigned short* q_s = (DEC_LDS unsigned short*)lds.q;
    DEC_LDS float* red = (DEC_LDS float*)lds.red;

    stage_q_mfma<G, HD, SCALED>(q, q_stride, scale, b, kvh, q_s, red, ksc);
    __syncthreads();
    typename kfrag_of<KVT>::type bq[HD / 32];
    build_qfrags<G, HD, KVT>(q_s, lg, li, bq);

    const int* bt = block_table + (long)b * W;
    // loop chunks with stride gridDim.z: the q staging amortizes and the
    // per-chunk softmax tail overlaps other chunks' K bursts (single-chunk
    // blocks measured ~66% memory-idle from cold-start/tail phases)
    for (int chunk = blk.c0 + blockIdx.z; chunk * DEC_CHUNK < L;
         chunk += gridDim.z) {
    const int wave_key0 = chunk * DEC_CHUNK + wid * WAVE;  // 64 keys per wave
    float sv[TILES * 4];
    mfma_scores_softmax<G, HD, KVT, SCALED, WINDOWED, false>(
        blk, k_cache, nkv, bs, ksc, bq, wave_key0, wid, lg, li, red, bt, 0, sv);

    // p write-out: [key][G]; lanes with the same (t, r) write G consecutive
    // floats for 4 key-groups -> 4 x 64 B segments per instruction
    if (li < G) {
        unsigned short* pbase =
            p_out + (((long)b * nkv + kvh) * C + chunk) * DEC_CHUNK * G;
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = wid * WAVE + t * 16 + lg * 4 + r;
                pbase[key * G + li] = f2bf(sv[t * 4 + r]);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* pml = part_ml + ((((long)b * nkv + kvh) * C + chunk) * G) * 2;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float mc, lc;
            chunk_ml<G>(red, g, mc, lc);
            pml[g * 2] = mc;
            pml[g * 2 + 1] = lc;
        }
    }
    __syncthreads();  // red reused by the next chunk iteration
    }  // chunk loop
}

// ----------------------------------------------------------- stage 2: PV
// When FOLD (launcher sets it iff gridDim.z == 1, i.e. every chunk of this
// (b, kvh) runs serially in THIS workgroup — always true at flagship batch
// sizes where B*nkv >= 4096), the kernel carries the running flash-decoding
// merge (M, l, acc) across chunks in LDS (see fold_init) and writes the
// normalized bf16 output directly: no part_o round-trip, no combine kernel.
// PV_LOOP: the V loop is written out here and again in the fused kernel.
// As a shared stage (by reference, by value, with LDS-typed or plain
// pointers, with a sched_barrier) it cost 17 of the 96 hd-64 fused
// instantiations with G 1-8 one to six VGPRs across the 80-VGPR edge, 6 -> 5
// waves/SIMD, and this kernel a wave at G 16; in place, both keep the
// parent's figures for G 1-8. Change the two copies together.
template <int G, bool FOLD, typename KVT, bool WINDOWED>
__global__ __launch_bounds__(DEC_BLOCK) void attn_pv_kernel(
    const KVT* __restrict__ v_cache,             // [nb, nkv, bs, hd]
    const int* __restrict__ block_table,
    const int* __restrict__ seq_lens,
    const unsigned short* __restrict__ p_in,     // [B,nkv,C,CHUNK,G] bf16
    float* __restrict__ part_o,                  // [B, nkv, C, G, hd]
    const float* __restrict__ part_ml,           // [B, nkv, C, G, 2]
    unsigned short* __restrict__ out,            // [B, nq, hd] (FOLD only)
    float* __restrict__ out_ml,                  // optional [B, nq, 2]:
                                                 // final (m, l) per q head —
                                                 // the cross-rank merge
                                                 // state for context
                                                 // parallelism (parallel/cp)
    int nkv, int W, int bs, int hd, int C,
    const float* __restrict__ v_scale,           // [nkv] or nullptr
    int window) {                                // read iff WINDOWED
    const DecBlock<WINDOWED> blk(seq_lens, window);
    if (blk.idle()) return;
    const int b = blk.b, kvh = blk.kvh, L = blk.L;
    const int lane = threadIdx.x % WAVE;
    const int wid = threadIdx.x / WAVE;
    const bool scaled = sizeof(KVT) == 1 && v_scale != nullptr;
    const float vsc = scaled ? v_scale[kvh] : 1.f;

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const auto lds = pv_lds((DEC_LDS char*)smem_raw, G, hd);
    DEC_LDS float* p_s = (DEC_LDS float*)lds.p;
    DEC_LDS long* voff_s = (DEC_LDS long*)lds.voff;
    DEC_LDS float* merge = (DEC_LDS float*)lds.merge;
    DEC_LDS float* run = (DEC_LDS float*)lds.run;
    DEC_LDS float* runml = (DEC_LDS float*)lds.runml;
    if (FOLD) fold_init<G>(run, runml, hd, lane, wid);

    for (int chunk = blk.c0 + blockIdx.z; chunk * DEC_CHUNK < L;
         chunk += gridDim.z) {
    const int start = chunk * DEC_CHUNK;
    // stage p for the whole chunk into LDS, widening bf16 -> fp32 so the
    // inner fma loop reads full-rate f32x4
    {
        const unsigned short* psrc =
            p_in + (((long)b * nkv + kvh) * C + chunk) * DEC_CHUNK * G;
        for (int i = threadIdx.x; i < DEC_CHUNK * G / 8; i += DEC_BLOCK) {
            float v[8];
            load_bf16x8(psrc + i * 8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) p_s[i * 8 + j] = v[j];
        }
    }
    // per-thread V row offset (one chained block-table load per key)
    {
        const int* bt = block_table + (long)b * W;
        const int key = start + threadIdx.x;
        long voff = 0;
        if (blk.live(key))
            voff = kv_row_off(bt[key / bs], nkv, kvh, bs, key, hd);
        voff_s[threadIdx.x] = voff;
    }
    __syncthreads();

    const int wave_start = wid * WAVE;
    const int nkeys = min(WAVE, L - (start + wave_start));
    const int kfirst =
        WINDOWED ? min(WAVE, max(0, blk.lo - (start + wave_start))) : 0;
    // PV for this wave's 64-key slice: accumulates the live keys [kfirst,
    // nkeys) (kfirst > 0 only where the window's lower edge falls inside the
    // slice: V rows below it are never loaded); the lane owns output dims
    // (d0, d0+1). PV_LOOP: this block is written out in attn_pv_kernel and
    // in attn_decode_fused_kernel, the same text but for the head size, and
    // not as a shared stage: see the note above attn_pv_kernel.
    const int d0 = lane * 2;
    float o0[G], o1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) o0[g] = o1[g] = 0.f;
    if (d0 < hd && nkeys > kfirst) {
        const DEC_LDS long* voffs = voff_s + wave_start;
        const DEC_LDS float* pw = p_s + wave_start * G;
        int t = kfirst;
        for (; t + 32 <= nkeys; t += 32) {  // 32 V loads in flight
            kv_pair_t<KVT> vv[32];
#pragma unroll
            for (int j = 0; j < 32; ++j)
                vv[j] = load_v_pair<KVT>(v_cache + voffs[t + j] + d0);
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const float2v vf = kv_pair_f32(vv[j]);
                const DEC_LDS float* pt = pw + (t + j) * G;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    o0[g] = fmaf(pt[g], vf.x, o0[g]);
                    o1[g] = fmaf(pt[g], vf.y, o1[g]);
                }
            }
        }
        for (; t < nkeys; ++t) {
            const kv_pair_t<KVT> vv =
                load_v_pair<KVT>(v_cache + voffs[t] + d0);
            const float2v vf = kv_pair_f32(vv);
            const DEC_LDS float* pt = pw + t * G;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                o0[g] = fmaf(pt[g], vf.x, o0[g]);
                o1[g] = fmaf(pt[g], vf.y, o1[g]);
            }
        }
    }

    const long base = (((long)b * nkv + kvh) * C + chunk) * G;
    // FOLD: online merge with this chunk's (m, l) from the scores pass
    merge_chunk<G, FOLD, false>(o0, o1, hd, lane, wid, merge, run, runml,
                                part_o, nullptr, part_ml, nullptr, base,
                                scaled, vsc);
    __syncthreads();  // LDS buffers reused by the next chunk iteration
    }  // chunk loop

    if (FOLD)
        fold_epilogue<G>(run, runml, out, out_ml, b, kvh, nkv, hd, lane, wid,
                         scaled, vsc);
}

// ------------------------------------------------------ stage 3: combine
template <int G, bool WINDOWED>
__global__ __launch_bounds__(DEC_BLOCK) void attn_decode_combine_kernel(
    const float* __restrict__ part_o,   // [B, nkv, C, G, hd]
    const float* __restrict__ part_ml,  // [B, nkv, C, G, 2]
    const int* __restrict__ seq_lens,
    unsigned short* __restrict__ out,   // [B, nq, hd]
    float* __restrict__ out_ml,         // optional [B, nq, 2] (see PV)
    int nkv, int hd, int C,
    int window) {                       // read iff WINDOWED
    const int b = blockIdx.x;
    const int kvh = blockIdx.y;
    const int g = blockIdx.z;  // one block per (seq, kv head, q head)
    const int nq = nkv * G;
    const int L = seq_lens[b];
    const int nc = (L + DEC_CHUNK - 1) / DEC_CHUNK;
    // chunks wholly below the window were never produced: walk c0..nc
    const int c0 = WINDOWED ? max(0, L - window) / DEC_CHUNK : 0;
    const long base = ((long)b * nkv + kvh) * C;

    // stage this head's (m, l) pairs once
    __shared__ float ml_s[DEC_MAX_CHUNKS][2];
    for (int c = c0 + threadIdx.x; c < nc; c += DEC_BLOCK) {
        ml_s[c][0] = part_ml[((base + c) * G + g) * 2];
        ml_s[c][1] = part_ml[((base + c) * G + g) * 2 + 1];
    }
    __syncthreads();
    float M = -1e30f;
    for (int c = c0; c < nc; ++c) M = fmaxf(M, ml_s[c][0]);
    float Ltot = 0.f;
    for (int c = c0; c < nc; ++c) Ltot += __expf(ml_s[c][0] - M) * ml_s[c][1];
    const float inv = (Ltot > 0.f) ? 1.f / Ltot : 0.f;
    if (out_ml != nullptr && threadIdx.x == 0) {
        float* mlrow = out_ml + ((long)b * nq + kvh * G + g) * 2;
        mlrow[0] = M;
        mlrow[1] = Ltot;
    }

    for (int d = threadIdx.x; d < hd; d += DEC_BLOCK) {
        float acc = 0.f;
        for (int c = c0; c < nc; ++c)
            acc += __expf(ml_s[c][0] - M) *
                   part_o[((base + c) * G + g) * hd + d];
        out[((long)b * nq + kvh * G + g) * hd + d] = f2bf(acc * inv);
    }
}

// ------------------------------------------- fused scores + PV (hd 64/128)
// The stages of attn_scores_mfma_kernel and attn_pv_kernel composed in one
// launch: per chunk the block runs mfma_scores_softmax, leaves p in LDS in
// the [key][G] fp32 layout the V loop reads, and goes straight on to the V
// loop (PV_LOOP, the one piece written out twice) and merge_chunk. The
// stages are the very functions the split kernels call and the V loop is
// the same text, so out / out_ml (and part_o / part_ml without FOLD) are
// bit for bit what the two kernels produce. What the fusion drops:
//   - the bf16 p scratch round trip through HBM and the part_ml re-read;
//   - the second launch with its own fill/drain and seq_lens / block-table
//     reads: a key's page is looked up once by the thread that owns the key
//     and reaches the K-fragment rows by a wave shuffle (K and V caches
//     share one layout, so the same page serves the V row offset);
//   - the single-thread (m, l) tail: the wave that owns head g reduces the
//     chunk's (m, l) from `red` itself at fold time (chunk_ml, same order
//     of sums).
// LDS: fused_lds, the PV kernel's layout, then q_s and red (q_s is dead
// once the B fragments are built).
// The two phases run one after the other and each fits 4 waves/SIMD on its
// own, but nothing tells the compiler so: left alone it allocated 285
// registers, and with the occupancy asked for it kept every lane-derived
// index and the B fragments live across the PV loop and spilled them. So
// each phase derives its indices from phase_tid(), a thread id the
// optimizer cannot see through, and the B fragments are rebuilt from q_s
// every chunk: nothing but scalars lives from one phase to the next.
__device__ __forceinline__ int phase_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

template <int G, int HD, bool FOLD, typename KVT, bool SCALED, bool WINDOWED>
__global__ __launch_bounds__(DEC_BLOCK)
__attribute__((amdgpu_waves_per_eu(4))) void attn_decode_fused_kernel(
    const unsigned short* __restrict__ q,        // [B, nq, HD] (strided)
    const KVT* __restrict__ k_cache,             // [nb, nkv, bs, HD]
    const KVT* __restrict__ v_cache,             // [nb, nkv, bs, HD]
    const int* __restrict__ block_table,         // [B, W]
    const int* __restrict__ seq_lens,            // [B]
    float* __restrict__ part_o,                  // [B, nkv, C, G, HD] (!FOLD)
    float* __restrict__ part_ml,                 // [B, nkv, C, G, 2]  (!FOLD)
    unsigned short* __restrict__ out,            // [B, nq, HD] (FOLD)
    float* __restrict__ out_ml,                  // optional [B, nq, 2] (FOLD)
    int nkv, int W, int bs, int C, long q_stride, float scale,
    const float* __restrict__ k_scale,           // [nkv]; read iff SCALED
    const float* __restrict__ v_scale,           // [nkv]; read iff SCALED
    int window) {                                // read iff WINDOWED
    constexpr int TILES = WAVE / 16;
    const DecBlock<WINDOWED> blk(seq_lens, window);
    const int b = blk.b, kvh = blk.kvh, L = blk.L;
    if (blk.idle()) {
        // FOLD (gridDim.z == 1) owns the out rows: an empty sequence gets
        // what ops/reference.py returns, zeros and (m, l) = (-1e30, 0).
        // Without FOLD the combine kernel does the same.
        if (FOLD && L <= 0) {
            const int nq = nkv * G;
            unsigned short* orow = out + ((long)b * nq + kvh * G) * HD;
            for (int i = threadIdx.x; i < G * HD; i += DEC_BLOCK) orow[i] = 0;
            if (out_ml != nullptr && threadIdx.x < G) {
                float* mlrow =
                    out_ml + ((long)b * nq + kvh * G + threadIdx.x) * 2;
                mlrow[0] = -1e30f;
                mlrow[1] = 0.f;
            }
        }
        return;
    }
    float ksc = 1.f, vsc = 1.f;
    if (SCALED) {  // uniform: scalar loads
        ksc = k_scale[kvh];
        vsc = v_scale[kvh];
    }
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const auto lds = fused_lds((DEC_LDS char*)smem_raw, G, HD);
    DEC_LDS float* p_s = (DEC_LDS float*)lds.pv.p;
    DEC_LDS long* voff_s = (DEC_LDS long*)lds.pv.voff;
    DEC_LDS float* merge = (DEC_LDS float*)lds.pv.merge;
    DEC_LDS float* run = (DEC_LDS float*)lds.pv.run;
    DEC_LDS unsigned short* q_s = (DEC_LDS unsigned short*)lds.sc.q;
    DEC_LDS float* red = (DEC_LDS float*)lds.sc.red;
    DEC_LDS float* runml = (DEC_LDS float*)lds.runml;

    stage_q_mfma<G, HD, SCALED>(q, q_stride, scale, b, kvh, q_s, red, ksc);
    if (FOLD)
        fold_init<G>(run, runml, HD, threadIdx.x % WAVE, threadIdx.x / WAVE);
    __syncthreads();

    const int* bt = block_table + (long)b * W;
    for (int chunk = blk.c0 + blockIdx.z; chunk * DEC_CHUNK < L;
         chunk += gridDim.z) {
    const int start = chunk * DEC_CHUNK;
    {  // ---- scores phase
    const int tid = phase_tid();
    const int lane = tid % WAVE;
    const int wid = tid / WAVE;
    const int lg = lane >> 4;  // lane group 0..3
    const int li = lane & 15;
    const int wave_start = wid * WAVE;

    // addresses: thread t owns key start + t. One block-table lookup per
    // live key; a key past L or below the window is never looked up (its
    // entry may be stale) and keeps row offset 0.
    int page = 0;
    {
        const int key = start + tid;
        long voff = 0;
        if (blk.live(key)) {
            page = bt[key / bs];
            BB_KASSERT(page >= 0);  // block table row must be fully mapped
            voff = kv_row_off(page, nkv, kvh, bs, key, HD);
        }
        voff_s[tid] = voff;
    }

    // Rebuilt from q_s every chunk (KSTEPS LDS reads) so that they are not
    // live across the PV phase, which needs the registers.
    typename kfrag_of<KVT>::type bq[HD / 32];
    build_qfrags<G, HD, KVT>(q_s, lg, li, bq);

    // Row li of tile t is key wave_key0 + t*16 + li, owned by lane
    // t*16 + li of this wave: its page comes by shuffle.
    float sv[TILES * 4];
    mfma_scores_softmax<G, HD, KVT, SCALED, WINDOWED, true>(
        blk, k_cache, nkv, bs, ksc, bq, start + wave_start, wid, lg, li, red,
        nullptr, page, sv);

    // p stays in LDS, already bf16-rounded, widened for the fma loop
    if (li < G) {
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = wave_start + t * 16 + lg * 4 + r;
                p_s[key * G + li] = sv[t * 4 + r];
            }
        }
    }
    }  // scores phase
    __syncthreads();

    // ---- PV phase
    const int tid = phase_tid();
    const int lane = tid % WAVE;
    const int wid = tid / WAVE;
    const int wave_start = wid * WAVE;
    const int wave_key0 = start + wave_start;
    const int nkeys = min(WAVE, L - wave_key0);
    const int kfirst = WINDOWED ? min(WAVE, max(0, blk.lo - wave_key0)) : 0;
    // PV for this wave's 64-key slice: accumulates the live keys [kfirst,
    // nkeys) (kfirst > 0 only where the window's lower edge falls inside the
    // slice: V rows below it are never loaded); the lane owns output dims
    // (d0, d0+1). PV_LOOP: this block is written out in attn_pv_kernel and
    // in attn_decode_fused_kernel, the same text but for the head size, and
    // not as a shared stage: see the note above attn_pv_kernel.
    const int d0 = lane * 2;
    float o0[G], o1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) o0[g] = o1[g] = 0.f;
    if (d0 < HD && nkeys > kfirst) {
        const DEC_LDS long* voffs = voff_s + wave_start;
        const DEC_LDS float* pw = p_s + wave_start * G;
        int t = kfirst;
        for (; t + 32 <= nkeys; t += 32) {  // 32 V loads in flight
            kv_pair_t<KVT> vv[32];
#pragma unroll
            for (int j = 0; j < 32; ++j)
                vv[j] = load_v_pair<KVT>(v_cache + voffs[t + j] + d0);
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const float2v vf = kv_pair_f32(vv[j]);
                const DEC_LDS float* pt = pw + (t + j) * G;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    o0[g] = fmaf(pt[g], vf.x, o0[g]);
                    o1[g] = fmaf(pt[g], vf.y, o1[g]);
                }
            }
        }
        for (; t < nkeys; ++t) {
            const kv_pair_t<KVT> vv =
                load_v_pair<KVT>(v_cache + voffs[t] + d0);
            const float2v vf = kv_pair_f32(vv);
            const DEC_LDS float* pt = pw + t * G;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                o0[g] = fmaf(pt[g], vf.x, o0[g]);
                o1[g] = fmaf(pt[g], vf.y, o1[g]);
            }
        }
    }

    // this chunk's (m, l) comes straight from `red` (wave-uniform LDS reads)
    merge_chunk<G, FOLD, true>(o0, o1, HD, lane, wid, merge, run, runml,
                               part_o, part_ml, nullptr, red,
                               (((long)b * nkv + kvh) * C + chunk) * G, SCALED,
                               vsc);
    __syncthreads();  // LDS buffers reused by the next chunk iteration
    }  // chunk loop

    if (FOLD) {
        const int tid = phase_tid();
        fold_epilogue<G>(run, runml, out, out_ml, b, kvh, nkv, HD, tid % WAVE,
                         tid / WAVE, SCALED, vsc);
    }
}

// ---------------------------------------------------------------- launch
// Which kernels a decode launch takes, for the launcher and for the caller
// that sizes the scratch: Z chunk-walkers per (b, kvh), and whether the
// fused scores + PV kernel runs. path: 0 = auto, 1 = split, 2 = fused (the
// caller rejects 2 for hd other than 64/128). max_z: 0 = the rule below,
// n = cap Z at n. Auto is fused per cache type where it was measured
// faster at the flagship shape (docs/KERNELS.md, "Fused scores + PV").
#define DEC_FUSED_AUTO_BF16 1
#define DEC_FUSED_AUTO_FP8 1
extern "C" void attn_decode_plan(int B, int nkv, int hd, int C, int fp8,
                                 int path, int max_z, int* Z_out,
                                 int* fused_out) {
    // enough blocks to fill the chip, but chunks loop within a block so the
    // cold-start/tail phases amortize over multiple 64 KB K/V bursts
    int Z = (4096 + B * nkv - 1) / (B * nkv);
    if (Z > C) Z = C;
    if (max_z > 0 && Z > max_z) Z = max_z;
    if (Z < 1) Z = 1;
    *Z_out = Z;
    const bool can = hd == 64 || hd == 128;
    if (path == 0)
        *fused_out =
            can && (fp8 ? DEC_FUSED_AUTO_FP8 : DEC_FUSED_AUTO_BF16);
    else
        *fused_out = path == 2 && can;
}

namespace {

// launch_attn_decode's arguments plus the plan, handed down the dispatch
struct DecodeArgs {
    const unsigned short* q;
    const void *k_cache, *v_cache;
    const int *block_table, *seq_lens;
    unsigned short* p_buf;
    float *part_o, *part_ml;
    unsigned short* out;
    float* out_ml;
    int nkv, W, bs, hd, C;
    long q_stride;
    float scale;
    const float *k_scale, *v_scale;
    int window;
    bool fused;
    dim3 grid;   // (B, nkv, Z)
    dim3 cgrid;  // (B, nkv, G)
    hipStream_t stream;
};

// runtime G -> compile-time constant; ext.cpp admits no other group size
template <typename F>
void with_group(int G, F f) {
    switch (G) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        // 7: Qwen2.5-7B, 28 q / 4 kv heads
        case 7: f(std::integral_constant<int, 7>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
    }
}

// SCALED only exists for the fp8 cache type
template <typename KVT, typename F>
void with_scaled(const float* k_scale, F f) {
    if constexpr (sizeof(KVT) == 1) {
        if (k_scale != nullptr) {
            f(std::true_type{});
            return;
        }
    }
    f(std::false_type{});
}

template <int G, int HD, typename KVT, bool WIN>
void launch_scores_mfma(const DecodeArgs& a) {
    with_scaled<KVT>(a.k_scale, [&](auto scaled) {
        hipLaunchKernelGGL(
            (attn_scores_mfma_kernel<G, HD, KVT, decltype(scaled)::value, WIN>),
            a.grid,
            dim3(DEC_BLOCK), scores_lds(0, G, HD).end, a.stream, a.q,
            static_cast<const KVT*>(a.k_cache), a.block_table, a.seq_lens,
            a.p_buf, a.part_ml, a.nkv, a.W, a.bs, a.C, a.q_stride, a.scale,
            a.k_scale, a.window);
    });
}

// FOLD iff one block walks every chunk of its (b, kvh)
template <int G, int HD, typename KVT, bool WIN>
void launch_fused(const DecodeArgs& a) {
    with_scaled<KVT>(a.k_scale, [&](auto scaled) {
        constexpr bool SC = decltype(scaled)::value;
        hipLaunchKernelGGL(
            (a.grid.z == 1
                 ? attn_decode_fused_kernel<G, HD, true, KVT, SC, WIN>
                 : attn_decode_fused_kernel<G, HD, false, KVT, SC, WIN>),
            a.grid, dim3(DEC_BLOCK), fused_lds(0, G, HD).end, a.stream, a.q,
            static_cast<const KVT*>(a.k_cache),
            static_cast<const KVT*>(a.v_cache), a.block_table, a.seq_lens,
            a.part_o, a.part_ml, a.out, a.out_ml, a.nkv, a.W, a.bs, a.C,
            a.q_stride, a.scale, a.k_scale, a.v_scale, a.window);
    });
}

// window > 0 selects the WINDOWED instantiations; window == 0 launches the
// same code as before the window existed (the flag folds lo and c0 to 0).
// The fused path reads neither p_buf nor, with Z == 1, part_o / part_ml.
template <int G, typename KVT, bool WIN>
void launch_decode(const DecodeArgs& a) {
    const int hd = a.hd;
    const bool fold = a.grid.z == 1;
    if (a.fused) {
        if (hd == 128) launch_fused<G, 128, KVT, WIN>(a);
        else launch_fused<G, 64, KVT, WIN>(a);
    } else {
        if (hd == 128) launch_scores_mfma<G, 128, KVT, WIN>(a);
        else if (hd == 64) launch_scores_mfma<G, 64, KVT, WIN>(a);
        else
            hipLaunchKernelGGL(
                (attn_scores_kernel<G, KVT, WIN>), a.grid, dim3(DEC_BLOCK),
                scores_lds(0, G, hd).end, a.stream, a.q,
                static_cast<const KVT*>(a.k_cache), a.block_table,
                a.seq_lens, a.p_buf, a.part_ml, a.nkv, a.W, a.bs, hd, a.C,
                a.q_stride, a.scale, a.k_scale, a.window);
        hipLaunchKernelGGL(
            (fold ? attn_pv_kernel<G, true, KVT, WIN>
                  : attn_pv_kernel<G, false, KVT, WIN>),
            a.grid, dim3(DEC_BLOCK), pv_lds(0, G, hd).end, a.stream,
            static_cast<const KVT*>(a.v_cache), a.block_table, a.seq_lens,
            a.p_buf, a.part_o, a.part_ml, a.out, fold ? a.out_ml : nullptr,
            a.nkv, a.W, a.bs, hd, a.C, a.v_scale, a.window);
    }
    if (!fold)
        hipLaunchKernelGGL((attn_decode_combine_kernel<G, WIN>), a.cgrid,
                           dim3(DEC_BLOCK), 0, a.stream, a.part_o, a.part_ml,
                           a.seq_lens, a.out, a.out_ml, a.nkv, hd, a.C,
                           a.window);
}

}  // namespace

// window > 0: sliding-window attention, keys [max(0, L - window), L) are
// live.
extern "C" void launch_attn_decode(
    const unsigned short* q, const void* k_cache, const void* v_cache,
    const int* block_table, const int* seq_lens, unsigned short* p_buf,
    float* part_o, float* part_ml, unsigned short* out, float* out_ml,
    int B, int nkv,
    int G, int W, int bs, int hd, int C, long q_stride, float scale,
    int fp8, const float* k_scale, const float* v_scale, int window,
    int path, int max_z, hipStream_t stream) {
    int Z, fused;
    attn_decode_plan(B, nkv, hd, C, fp8, path, max_z, &Z, &fused);
    const DecodeArgs a{q, k_cache, v_cache, block_table, seq_lens, p_buf,
                       part_o, part_ml, out, out_ml, nkv, W, bs, hd, C,
                       q_stride, scale, k_scale, v_scale, window, fused != 0,
                       dim3(B, nkv, Z), dim3(B, nkv, G), stream};
    with_group(G, [&](auto g) {
        constexpr int GG = decltype(g)::value;
        if (window > 0) {
            if (fp8) launch_decode<GG, unsigned char, true>(a);
            else launch_decode<GG, unsigned short, true>(a);
        } else {
            if (fp8) launch_decode<GG, unsigned char, false>(a);
            else launch_decode<GG, unsigned short, false>(a);
        }
    });
}
