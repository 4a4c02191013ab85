// Torch bindings for the bee2bee_amd CDNA4 kernel set.
//
// Validation lives here (shape/dtype/device checks) so the kernels stay
// branch-free. All entry points are hipGraph-capture safe: no allocation
// beyond torch's caching allocator, no synchronization, no host reads.
// Every launch is followed by check_launch, and an empty grid never launches.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "attn_decode.h"

using torch::Tensor;

extern "C" {
void launch_rmsnorm(const unsigned short*, const unsigned short*,
                    unsigned short*, long, int, float, hipStream_t);
void launch_fused_add_rmsnorm(const unsigned short*, const unsigned short*,
                              const unsigned short*, unsigned short*,
                              unsigned short*, long, int, float, hipStream_t);
void launch_layernorm(const unsigned short*, const unsigned short*,
                      const unsigned short*, unsigned short*, long, int,
                      float, hipStream_t);
void launch_fused_add_layernorm(const unsigned short*, const unsigned short*,
                                const unsigned short*, const unsigned short*,
                                unsigned short*, unsigned short*, long, int,
                                float, hipStream_t);
void launch_gelu(const unsigned short*, unsigned short*, long, hipStream_t);
void launch_rope(unsigned short*, unsigned short*, const int*, const float*,
                 const float*, int, int, int, int, long, long, hipStream_t);
void launch_qk_norm_rope(unsigned short*, unsigned short*, const int*,
                         const float*, const float*, const unsigned short*,
                         const unsigned short*, int, int, int, int, long,
                         long, float, hipStream_t);
void launch_kv_store(const unsigned short*, const unsigned short*,
                     unsigned short*, unsigned short*, const int*, int, int,
                     int, int, long, long, hipStream_t);
void launch_kv_store_fp8(const unsigned short*, const unsigned short*,
                         unsigned char*, unsigned char*, const int*,
                         const float*, const float*, int, int, int, int, long,
                         long, hipStream_t);
void launch_rope_kv_store(unsigned short*, unsigned short*,
                          const unsigned short*, void*, void*, const int*,
                          const int*, const float*, const float*, const float*,
                          const float*, int, int, int, int, int, int, long,
                          long, long, hipStream_t);
void launch_swiglu(const unsigned short*, unsigned short*, long, long,
                   hipStream_t);
void launch_attn_prefill(const unsigned short*, const unsigned short*,
                         const unsigned short*, const int*, unsigned short*,
                         int, int, int, int, long, long, long, int, float,
                         int, int, hipStream_t);
void launch_attn_prefill_paged(const unsigned short*, const void*,
                               const void*, const int*, const int*,
                               const int*, unsigned short*, int, int, int,
                               int, long, int, int, int, float, int,
                               const float*, const float*, int, hipStream_t);
void launch_mfma_probe(const unsigned short*, const unsigned short*, float*,
                       hipStream_t);
void launch_mfma_probe_fp8(const unsigned char*, const unsigned char*,
                           float*, hipStream_t);
void launch_grouped_gemm(const unsigned short*, const unsigned short*,
                         const int*, unsigned short*, int, int, int, int,
                         hipStream_t);
void launch_bw_linear(const unsigned short*, long, float*, hipStream_t);
void launch_bw_rowperlane(const unsigned short*, long, int, int, int, float*,
                          hipStream_t);
void launch_bw_rowperinstr(const unsigned short*, long, int, int, int, float*,
                           hipStream_t);
void launch_bw_paged(const unsigned short*, const int*, long, int, int, int,
                     float*, hipStream_t);
void launch_sample_rows(const void*, int, long, int, int, const float*,
                        const int*, const float*, const float*,
                        const unsigned char*, long, int, const int*,
                        const long long*, const int*, long long*,
                        hipStream_t);
}

namespace {

inline hipStream_t stream() {
    return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

inline bool hd_fp8_ok(long hd) { return hd % 8 == 0; }

using OptTensor = c10::optional<Tensor>;

// Per-kv-head fp8 scales: both given or neither; fp32 [nkv] contiguous on
// the cache's device; only meaningful for a uint8 (fp8) cache. Returns
// true when scales are present.
bool check_kv_scales(const OptTensor& a, const OptTensor& b,
                     const Tensor& cache, const char* what) {
    TORCH_CHECK(a.has_value() == b.has_value(), what,
                ": give both K and V scales or neither");
    if (!a.has_value()) return false;
    TORCH_CHECK(cache.scalar_type() == torch::kUInt8, what,
                ": per-head KV scales need an fp8 (uint8) cache");
    for (const Tensor* t : {&*a, &*b}) {
        TORCH_CHECK(t->is_cuda() && t->device() == cache.device(), what,
                    ": scales must be on the cache's device");
        TORCH_CHECK(t->scalar_type() == torch::kFloat32 && t->dim() == 1 &&
                        t->size(0) == cache.size(1) && t->is_contiguous(),
                    what, ": scales must be fp32 [n_kv_heads] contiguous");
    }
    return true;
}

inline const unsigned short* bf16p(const Tensor& t) {
    return reinterpret_cast<const unsigned short*>(t.data_ptr());
}

inline unsigned short* bf16p_mut(Tensor& t) {
    return reinterpret_cast<unsigned short*>(t.data_ptr());
}

void check_bf16(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
}

// Follows every launch: a launch the runtime refuses (too much dynamic LDS,
// an empty or oversized grid) would otherwise hand back torch::empty memory.
// hipGetLastError reads and clears a host-side status: no synchronization,
// legal under stream capture, and never executed by a graph replay.
void check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    TORCH_CHECK(e == hipSuccess, what, ": HIP kernel launch failed: ",
                hipGetErrorString(e));
}

// The row-norm kernels cache one fp32 row in dynamic LDS (H * 4 bytes) next
// to 64 bytes of static reduction scratch. Returns H after checking it and
// the [H] bf16 parameter vectors.
int check_norm_row(const Tensor& x, const char* what,
                   std::initializer_list<const Tensor*> params) {
    TORCH_CHECK(x.dim() >= 1, what, ": x needs at least one dimension");
    const long H = x.size(-1);
    TORCH_CHECK(H > 0 && H % 8 == 0, what,
                ": hidden size must be a positive multiple of 8, got ", H);
    const long lds = (long)at::cuda::getCurrentDeviceProperties()
                         ->sharedMemPerBlock;
    const long h_max = (lds - 64) / 4 / 8 * 8;
    TORCH_CHECK(H <= h_max, what, ": hidden size ", H, " needs ", H * 4 + 64,
                " bytes of LDS per workgroup; the device limit is ", lds,
                " bytes (hidden size <= ", h_max, ")");
    for (const Tensor* p : params) {
        check_bf16(*p, "norm weight/bias");
        TORCH_CHECK(p->dim() == 1 && p->size(0) == H && p->is_contiguous(),
                    what, ": weight and bias must be bf16 [", H,
                    "] contiguous");
    }
    return (int)H;
}

Tensor rmsnorm(const Tensor& x, const Tensor& w, double eps) {
    check_bf16(x, "x");
    TORCH_CHECK(x.is_contiguous());
    const int H = check_norm_row(x, "rmsnorm", {&w});
    const long T = x.numel() / H;
    Tensor y = torch::empty_like(x);
    if (T == 0) return y;
    launch_rmsnorm(bf16p(x), bf16p(w), bf16p_mut(y), T, H, (float)eps,
                   stream());
    check_launch("rmsnorm");
    return y;
}

std::vector<Tensor> fused_add_rmsnorm(const Tensor& x, const Tensor& resid,
                                      const Tensor& w, double eps) {
    check_bf16(x, "x");
    check_bf16(resid, "resid");
    TORCH_CHECK(x.is_contiguous() && resid.is_contiguous());
    TORCH_CHECK(x.sizes() == resid.sizes());
    const int H = check_norm_row(x, "fused_add_rmsnorm", {&w});
    const long T = x.numel() / H;
    Tensor y = torch::empty_like(x);
    Tensor resid_out = torch::empty_like(x);
    if (T == 0) return {y, resid_out};
    launch_fused_add_rmsnorm(bf16p(x), bf16p(resid), bf16p(w), bf16p_mut(y),
                             bf16p_mut(resid_out), T, H, (float)eps, stream());
    check_launch("fused_add_rmsnorm");
    return {y, resid_out};
}

struct RopeDims { int T, nq, nkv, hd; };

// Every check of rope_inplace; rope_kv_store makes the same ones.
RopeDims check_rope_args(const Tensor& q, const Tensor& k, const Tensor& pos,
                         const Tensor& cos_t, const Tensor& sin_t) {
    check_bf16(q, "q");
    check_bf16(k, "k");
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && k.device() == q.device(),
                "rope: q and k must be [T, heads, head_dim] on one device");
    TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == torch::kInt32 &&
                    pos.dim() == 1 && pos.is_contiguous(),
                "rope: positions must be int32 [T] contiguous on GPU");
    TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda() &&
                    cos_t.scalar_type() == torch::kFloat32 &&
                    sin_t.scalar_type() == torch::kFloat32,
                "rope: cos/sin tables must be fp32 on GPU");
    const int T = q.size(0);
    const int nq = q.size(1), nkv = k.size(1), hd = q.size(2);
    TORCH_CHECK(hd >= 2 && hd % 2 == 0,
                "rope: head_dim must be even and >= 2, got ", hd);
    TORCH_CHECK(k.size(2) == hd && k.size(0) == T,
                "rope: k must have q's token count and head_dim");
    TORCH_CHECK(pos.size(0) == T, "rope: need one position per token, got ",
                pos.size(0), " for ", T, " tokens");
    // heads/dims contiguous within a token; token stride may be larger
    TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == hd);
    TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == hd);
    TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == hd / 2 &&
                    cos_t.sizes() == sin_t.sizes() && cos_t.is_contiguous() &&
                    sin_t.is_contiguous(),
                "rope: cos and sin must both be [max_len, head_dim / 2] "
                "contiguous");
    TORCH_CHECK((long)T * (nq + nkv) <= INT_MAX);
    return {T, nq, nkv, hd};
}

void rope_inplace(Tensor& q, Tensor& k, const Tensor& pos, const Tensor& cos_t,
                  const Tensor& sin_t) {
    const auto [T, nq, nkv, hd] = check_rope_args(q, k, pos, cos_t, sin_t);
    if (T == 0 || nq + nkv == 0) return;
    launch_rope(bf16p_mut(q), bf16p_mut(k), pos.data_ptr<int>(),
                cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), T, nq, nkv,
                hd, q.stride(0), k.stride(0), stream());
    check_launch("rope");
}

// Qwen3 per-head q/k RMSNorm + RoPE, in place. Layout contract of
// rope_inplace, plus one bf16 [hd] norm weight each for q and k.
void qk_norm_rope_inplace(Tensor& q, Tensor& k, const Tensor& pos,
                          const Tensor& cos_t, const Tensor& sin_t,
                          const Tensor& q_weight, const Tensor& k_weight,
                          double eps) {
    check_bf16(q, "q");
    check_bf16(k, "k");
    check_bf16(q_weight, "q_weight");
    check_bf16(k_weight, "k_weight");
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3,
                "qk_norm_rope: q and k must be [T, heads, head_dim]");
    TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == torch::kInt32 &&
                    pos.dim() == 1 && pos.is_contiguous(),
                "qk_norm_rope: positions must be int32 [T] on GPU");
    TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda() &&
                    cos_t.scalar_type() == torch::kFloat32 &&
                    sin_t.scalar_type() == torch::kFloat32,
                "qk_norm_rope: cos/sin tables must be fp32 on GPU");
    const int T = q.size(0);
    const int nq = q.size(1), nkv = k.size(1), hd = q.size(2);
    TORCH_CHECK(hd >= 2 && hd % 2 == 0 && hd <= 256,
                "qk_norm_rope: head_dim must be even and <= 256, got ", hd);
    TORCH_CHECK(k.size(2) == hd && k.size(0) == T && pos.size(0) == T);
    // heads/dims contiguous within a token; token stride may be larger
    TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == hd);
    TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == hd);
    TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == hd / 2 &&
                cos_t.sizes() == sin_t.sizes() && cos_t.is_contiguous() &&
                sin_t.is_contiguous());
    for (const Tensor* w : {&q_weight, &k_weight})
        TORCH_CHECK(w->dim() == 1 && w->size(0) == hd && w->is_contiguous(),
                    "qk_norm_rope: norm weights must be bf16 [head_dim] "
                    "contiguous");
    TORCH_CHECK((long)T * (nq + nkv) <= INT_MAX);
    if (T == 0 || nq + nkv == 0) return;
    launch_qk_norm_rope(bf16p_mut(q), bf16p_mut(k), pos.data_ptr<int>(),
                        cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                        bf16p(q_weight), bf16p(k_weight), T, nq, nkv, hd,
                        q.stride(0), k.stride(0), (float)eps, stream());
    check_launch("qk_norm_rope");
}

struct StoreDims { int T, nkv, hd, bs; bool scaled; };

// Every check of kv_cache_store that stands before its early return for an
// empty call; rope_kv_store makes the same ones.
StoreDims check_kv_store_args(const Tensor& k, const Tensor& v,
                              const Tensor& k_cache, const Tensor& v_cache,
                              const Tensor& slots,
                              const OptTensor& k_inv_scale,
                              const OptTensor& v_inv_scale) {
    check_bf16(k, "k");
    check_bf16(v, "v");
    TORCH_CHECK(k.dim() == 3 && v.sizes() == k.sizes() &&
                    v.device() == k.device(),
                "kv_cache_store: k and v must both be [T, n_kv_heads, "
                "head_dim] on one device");
    TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
                    v_cache.scalar_type() == k_cache.scalar_type() &&
                    k_cache.device() == k.device() &&
                    v_cache.device() == k.device(),
                "kv_cache_store: the caches must be [n_blocks, n_kv_heads, "
                "block_size, head_dim], alike in size and dtype, on k's "
                "device");
    const bool scaled =
        check_kv_scales(k_inv_scale, v_inv_scale, k_cache, "kv_cache_store");
    const int T = k.size(0), nkv = k.size(1), hd = k.size(2);
    TORCH_CHECK(slots.is_cuda() && slots.device() == k.device() &&
                    slots.scalar_type() == torch::kInt32 &&
                    slots.dim() == 1 && slots.is_contiguous() &&
                    slots.size(0) == T,
                "kv_cache_store: slots must be int32 [T] contiguous on k's "
                "device, T = ", T);
    const int bs = k_cache.size(2);
    TORCH_CHECK(k_cache.size(1) == nkv && k_cache.size(3) == hd,
                "kv_cache_store: the caches' n_kv_heads and head_dim must "
                "be k's");
    TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
    TORCH_CHECK((long)T * nkv <= INT_MAX);
    TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == hd);
    TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == hd);
    TORCH_CHECK(hd % 2 == 0);
    return {T, nkv, hd, bs, scaled};
}

// The checks of a store that has tokens to write.
void check_kv_store_target(const Tensor& k_cache) {
    TORCH_CHECK(k_cache.numel() > 0,
                "kv_cache_store: tokens to store but an empty cache");
    if (k_cache.scalar_type() != torch::kUInt8) check_bf16(k_cache, "k_cache");
}

void launch_kv_store_any(const Tensor& k, const Tensor& v, Tensor& k_cache,
                         Tensor& v_cache, const Tensor& slots,
                         const OptTensor& k_inv_scale,
                         const OptTensor& v_inv_scale, const StoreDims& d) {
    if (k_cache.scalar_type() == torch::kUInt8) {
        // fp8 (OCP e4m3) cache: quantize at store time
        launch_kv_store_fp8(
            bf16p(k), bf16p(v), k_cache.data_ptr<unsigned char>(),
            v_cache.data_ptr<unsigned char>(), slots.data_ptr<int>(),
            d.scaled ? k_inv_scale->data_ptr<float>() : nullptr,
            d.scaled ? v_inv_scale->data_ptr<float>() : nullptr, d.T, d.nkv,
            d.hd, d.bs, k.stride(0), v.stride(0), stream());
    } else {
        launch_kv_store(bf16p(k), bf16p(v), bf16p_mut(k_cache),
                        bf16p_mut(v_cache), slots.data_ptr<int>(), d.T, d.nkv,
                        d.hd, d.bs, k.stride(0), v.stride(0), stream());
    }
    check_launch("kv_cache_store");
}

void kv_cache_store(const Tensor& k, const Tensor& v, Tensor& k_cache,
                    Tensor& v_cache, const Tensor& slots,
                    const OptTensor& k_inv_scale,
                    const OptTensor& v_inv_scale) {
    const StoreDims d = check_kv_store_args(k, v, k_cache, v_cache, slots,
                                            k_inv_scale, v_inv_scale);
    if (d.T == 0 || d.nkv == 0) return;
    check_kv_store_target(k_cache);
    launch_kv_store_any(k, v, k_cache, v_cache, slots, k_inv_scale,
                        v_inv_scale, d);
}

inline bool aligned16(const Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// rope_inplace(q, k, ...) followed by kv_cache_store(k, v, ...) as one
// call: every check of both stands before any launch. One fused kernel
// where the layout allows 16-byte lane accesses (head_dim % 16 == 0, token
// strides that are multiples of 8 elements, 16-byte-aligned bases); the two
// kernels of the separate ops otherwise, with the same result bit for bit.
void rope_kv_store(Tensor& q, Tensor& k, const Tensor& v, const Tensor& pos,
                   const Tensor& cos_t, const Tensor& sin_t, Tensor& k_cache,
                   Tensor& v_cache, const Tensor& slots,
                   const OptTensor& k_inv_scale,
                   const OptTensor& v_inv_scale) {
    const RopeDims r = check_rope_args(q, k, pos, cos_t, sin_t);
    const StoreDims d = check_kv_store_args(k, v, k_cache, v_cache, slots,
                                            k_inv_scale, v_inv_scale);
    TORCH_CHECK(q.device() == k_cache.device() &&
                    pos.device() == q.device() &&
                    cos_t.device() == q.device() &&
                    sin_t.device() == q.device(),
                "rope_kv_store: every tensor must be on one device");
    if (r.T == 0) return;
    if (d.nkv > 0) check_kv_store_target(k_cache);
    const long items = (long)(r.nq + 2 * r.nkv) * (r.hd / 16);
    const bool fast =
        d.nkv > 0 && r.hd % 16 == 0 && q.stride(0) % 8 == 0 &&
        k.stride(0) % 8 == 0 && v.stride(0) % 8 == 0 && aligned16(q) &&
        aligned16(k) && aligned16(v) && aligned16(k_cache) &&
        aligned16(v_cache) && aligned16(cos_t) && aligned16(sin_t) &&
        (long)r.T * items <= INT_MAX;
    if (!fast) {
        if (r.nq + r.nkv > 0) {
            launch_rope(bf16p_mut(q), bf16p_mut(k), pos.data_ptr<int>(),
                        cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), r.T,
                        r.nq, r.nkv, r.hd, q.stride(0), k.stride(0),
                        stream());
            check_launch("rope");
        }
        if (d.nkv > 0)
            launch_kv_store_any(k, v, k_cache, v_cache, slots, k_inv_scale,
                                v_inv_scale, d);
        return;
    }
    const int kind =
        k_cache.scalar_type() != torch::kUInt8 ? 0 : (d.scaled ? 2 : 1);
    launch_rope_kv_store(
        bf16p_mut(q), bf16p_mut(k), bf16p(v), k_cache.data_ptr(),
        v_cache.data_ptr(), pos.data_ptr<int>(), slots.data_ptr<int>(),
        cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
        d.scaled ? k_inv_scale->data_ptr<float>() : nullptr,
        d.scaled ? v_inv_scale->data_ptr<float>() : nullptr, kind, r.T, r.nq,
        r.nkv, r.hd, d.bs, q.stride(0), k.stride(0), v.stride(0), stream());
    check_launch("rope_kv_store");
}

Tensor layernorm(const Tensor& x, const Tensor& w, const Tensor& b,
                 double eps) {
    check_bf16(x, "x");
    TORCH_CHECK(x.is_contiguous());
    const int H = check_norm_row(x, "layernorm", {&w, &b});
    const long T = x.numel() / H;
    Tensor y = torch::empty_like(x);
    if (T == 0) return y;
    launch_layernorm(bf16p(x), bf16p(w), bf16p(b), bf16p_mut(y), T, H,
                     (float)eps, stream());
    check_launch("layernorm");
    return y;
}

std::vector<Tensor> fused_add_layernorm(const Tensor& x, const Tensor& resid,
                                        const Tensor& w, const Tensor& b,
                                        double eps) {
    check_bf16(x, "x");
    check_bf16(resid, "resid");
    TORCH_CHECK(x.is_contiguous() && resid.is_contiguous());
    TORCH_CHECK(x.sizes() == resid.sizes());
    const int H = check_norm_row(x, "fused_add_layernorm", {&w, &b});
    const long T = x.numel() / H;
    Tensor y = torch::empty_like(x);
    Tensor resid_out = torch::empty_like(x);
    if (T == 0) return {y, resid_out};
    launch_fused_add_layernorm(bf16p(x), bf16p(resid), bf16p(w), bf16p(b),
                               bf16p_mut(y), bf16p_mut(resid_out), T, H,
                               (float)eps, stream());
    check_launch("fused_add_layernorm");
    return {y, resid_out};
}

Tensor gelu(const Tensor& x) {
    check_bf16(x, "x");
    TORCH_CHECK(x.is_contiguous());
    TORCH_CHECK(x.numel() % 8 == 0);
    Tensor y = torch::empty_like(x);
    if (x.numel() == 0) return y;
    launch_gelu(bf16p(x), bf16p_mut(y), x.numel(), stream());
    check_launch("gelu");
    return y;
}

Tensor swiglu(const Tensor& gu) {
    check_bf16(gu, "gate_up");
    TORCH_CHECK(gu.is_contiguous());
    TORCH_CHECK(gu.dim() >= 1 && gu.size(-1) > 0 && gu.size(-1) % 16 == 0,
                "swiglu: the last dimension is 2 * I with I a positive "
                "multiple of 8");
    const long I = gu.size(-1) / 2;
    const long T = gu.numel() / gu.size(-1);
    // shaped like the input: [..., 2I] -> [..., I]
    std::vector<int64_t> shape(gu.sizes().begin(), gu.sizes().end());
    shape.back() = I;
    Tensor out = torch::empty(shape, gu.options());
    if (T == 0) return out;
    launch_swiglu(bf16p(gu), bf16p_mut(out), T, I, stream());
    check_launch("swiglu");
    return out;
}

std::vector<Tensor> attn_decode_impl(const Tensor& q, const Tensor& k_cache,
                                     const Tensor& v_cache,
                                     const Tensor& block_table,
                                     const Tensor& seq_lens, double scale,
                                     const OptTensor& k_scale,
                                     const OptTensor& v_scale,
                                     int64_t window, bool want_lse,
                                     int64_t path = 0, int64_t max_z = 0) {
    check_bf16(q, "q");
    TORCH_CHECK(path >= 0 && path <= 2,
                "attn_decode: path is 0 (auto), 1 (split) or 2 (fused)");
    TORCH_CHECK(max_z >= 0 && max_z <= INT_MAX,
                "attn_decode: max_z must be >= 0 (0 = no cap)");
    TORCH_CHECK(window >= 0 && window <= INT_MAX,
                "attn_decode: window must be >= 0 (0 = off)");
    const bool scaled =
        check_kv_scales(k_scale, v_scale, k_cache, "attn_decode");
    const bool fp8 = k_cache.scalar_type() == torch::kUInt8;
    if (!fp8) check_bf16(k_cache, "k_cache");
    TORCH_CHECK(fp8 ? hd_fp8_ok(q.size(2)) : true,
                "fp8 KV decode needs head_dim % 8 == 0");
    TORCH_CHECK(block_table.scalar_type() == torch::kInt32 &&
                seq_lens.scalar_type() == torch::kInt32);
    TORCH_CHECK(block_table.is_contiguous());
    const int B = q.size(0), nq = q.size(1), hd = q.size(2);
    const int nkv = k_cache.size(1), bs = k_cache.size(2);
    const int W = block_table.size(1);
    TORCH_CHECK(hd <= 128 && hd % 2 == 0, "decode kernel supports hd<=128");
    TORCH_CHECK(nq % nkv == 0);
    const int G = nq / nkv;
    TORCH_CHECK(G >= 1 && G <= 8 || G == 16,
                "unsupported GQA group size ", G);
    TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == hd);
    Tensor out = torch::empty({B, nq, hd}, q.options());
    // flash-decoding split: one partial per 256-key chunk, then combine
    const int C = (W * bs + DEC_CHUNK - 1) / DEC_CHUNK;
    TORCH_CHECK(C <= DEC_MAX_CHUNKS,
                "decode supports up to 32768-token contexts for now");
    TORCH_CHECK(path != 2 || hd == 64 || hd == 128,
                "attn_decode: the fused kernel supports head_dim 64 and 128, "
                "got ", hd);
    int Z = 1, fused = 0;
    attn_decode_plan(B, nkv, hd, C, fp8 ? 1 : 0, (int)path, (int)max_z, &Z,
                     &fused);
    auto fopt = q.options().dtype(torch::kFloat32);
    // the fused kernel keeps p in LDS, and with Z == 1 (FOLD) writes out
    // directly: no scratch at all
    Tensor p_buf, part_o, part_ml;
    if (!fused) p_buf = torch::empty({B, nkv, C, DEC_CHUNK, G}, q.options());
    if (!fused || Z > 1) {
        part_o = torch::empty({B, nkv, C, G, hd}, fopt);
        part_ml = torch::empty({B, nkv, C, G, 2}, fopt);
    }
    Tensor out_ml;
    float* out_ml_p = nullptr;
    if (want_lse) {
        out_ml = torch::empty({B, nq, 2}, fopt);
        out_ml_p = out_ml.data_ptr<float>();
    }
    if (B == 0 || nq == 0) {
        if (want_lse) return {out, out_ml};
        return {out};
    }
    launch_attn_decode(bf16p(q), k_cache.data_ptr(), v_cache.data_ptr(),
                       block_table.data_ptr<int>(), seq_lens.data_ptr<int>(),
                       p_buf.defined() ? bf16p_mut(p_buf) : nullptr,
                       part_o.defined() ? part_o.data_ptr<float>() : nullptr,
                       part_ml.defined() ? part_ml.data_ptr<float>() : nullptr,
                       bf16p_mut(out), out_ml_p, B, nkv, G, W, bs, hd, C,
                       q.stride(0), (float)scale, fp8 ? 1 : 0,
                       scaled ? k_scale->data_ptr<float>() : nullptr,
                       scaled ? v_scale->data_ptr<float>() : nullptr,
                       (int)window, (int)path, (int)max_z, stream());
    check_launch("attn_decode");
    if (want_lse) return {out, out_ml};
    return {out};
}

Tensor attn_decode(const Tensor& q, const Tensor& k_cache,
                   const Tensor& v_cache, const Tensor& block_table,
                   const Tensor& seq_lens, double scale,
                   const OptTensor& k_scale, const OptTensor& v_scale,
                   int64_t window) {
    return attn_decode_impl(q, k_cache, v_cache, block_table, seq_lens,
                            scale, k_scale, v_scale, window, false)[0];
}

// out + per-(seq, q-head) (m, l): the flash merge state that context
// parallelism exchanges across ranks (parallel/cp.py)
std::vector<Tensor> attn_decode_lse(const Tensor& q, const Tensor& k_cache,
                                    const Tensor& v_cache,
                                    const Tensor& block_table,
                                    const Tensor& seq_lens, double scale,
                                    const OptTensor& k_scale,
                                    const OptTensor& v_scale,
                                    int64_t window) {
    return attn_decode_impl(q, k_cache, v_cache, block_table, seq_lens,
                            scale, k_scale, v_scale, window, true);
}

// attn_decode_lse with the kernel path chosen by the caller: path 0 = auto,
// 1 = split (scores, PV, combine), 2 = fused scores + PV; max_z > 0 caps the
// chunk-walkers per (seq, kv head), so max_z = 1 forces the FOLD kernels.
// For tests and benchmarks; serving calls attn_decode / attn_decode_lse.
std::vector<Tensor> attn_decode_select(const Tensor& q, const Tensor& k_cache,
                                       const Tensor& v_cache,
                                       const Tensor& block_table,
                                       const Tensor& seq_lens, double scale,
                                       const OptTensor& k_scale,
                                       const OptTensor& v_scale,
                                       int64_t window, int64_t path,
                                       int64_t max_z) {
    return attn_decode_impl(q, k_cache, v_cache, block_table, seq_lens,
                            scale, k_scale, v_scale, window, true, path,
                            max_z);
}

Tensor attn_prefill(const Tensor& q, const Tensor& k, const Tensor& v,
                    const Tensor& cu_seqlens, long max_seqlen, double scale,
                    bool causal, int64_t window) {
    check_bf16(q, "q");
    check_bf16(k, "k");
    TORCH_CHECK(window >= 0 && window <= INT_MAX,
                "attn_prefill: window must be >= 0 (0 = off)");
    TORCH_CHECK(window == 0 || causal,
                "attn_prefill: a sliding window needs causal attention");
    TORCH_CHECK(cu_seqlens.scalar_type() == torch::kInt32 &&
                cu_seqlens.is_contiguous());
    const int T = q.size(0), nq = q.size(1), hd = q.size(2);
    const int nkv = k.size(1);
    const int nseq = cu_seqlens.size(0) - 1;
    TORCH_CHECK(nq % nkv == 0);
    // head dims other than the MFMA kernel's 64 / 128 take the basic
    // kernel: one lane per pair of dims, 64 lanes
    TORCH_CHECK(hd <= 128 && hd % 2 == 0,
                "attn_prefill: head_dim must be even and <= 128, got ", hd);
    TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == hd);
    TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == hd);
    TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == hd);
    Tensor out = torch::empty({T, nq, hd}, q.options());
    if (T == 0 || nq == 0 || nseq <= 0 || max_seqlen <= 0) return out;
    launch_attn_prefill(bf16p(q), bf16p(k), bf16p(v),
                        cu_seqlens.data_ptr<int>(), bf16p_mut(out), nseq, nq,
                        nkv, hd, q.stride(0), k.stride(0), v.stride(0),
                        (int)max_seqlen, (float)scale, causal ? 1 : 0,
                        (int)window, stream());
    check_launch("attn_prefill");
    return out;
}

Tensor attn_prefill_paged(const Tensor& q, const Tensor& k_cache,
                          const Tensor& v_cache, const Tensor& block_table,
                          const Tensor& seq_lens, const Tensor& cu_q,
                          long max_qlen, double scale,
                          const OptTensor& k_scale,
                          const OptTensor& v_scale, int64_t window) {
    check_bf16(q, "q");
    TORCH_CHECK(window >= 0 && window <= INT_MAX,
                "attn_prefill_paged: window must be >= 0 (0 = off)");
    const bool scaled =
        check_kv_scales(k_scale, v_scale, k_cache, "attn_prefill_paged");
    const bool fp8 = k_cache.scalar_type() == torch::kUInt8;
    if (!fp8) check_bf16(k_cache, "k_cache");
    TORCH_CHECK(block_table.scalar_type() == torch::kInt32 &&
                seq_lens.scalar_type() == torch::kInt32 &&
                cu_q.scalar_type() == torch::kInt32);
    TORCH_CHECK(block_table.is_contiguous() && cu_q.is_contiguous());
    const int T = q.size(0), nq = q.size(1), hd = q.size(2);
    const int nkv = k_cache.size(1), bs = k_cache.size(2);
    const int W = block_table.size(1);
    const int nseq = cu_q.size(0) - 1;
    TORCH_CHECK(nq % nkv == 0);
    TORCH_CHECK(hd % 8 == 0 && hd <= 128,
                "attn_prefill_paged: head_dim must be a multiple of 8 and "
                "<= 128, got ", hd);
    TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == hd);
    TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
    TORCH_CHECK(block_table.size(0) == nseq && seq_lens.size(0) == nseq);
    Tensor out = torch::empty({T, nq, hd}, q.options());
    if (T == 0 || nq == 0 || nseq <= 0 || max_qlen <= 0) return out;
    launch_attn_prefill_paged(bf16p(q), k_cache.data_ptr(),
                              v_cache.data_ptr(), cu_q.data_ptr<int>(),
                              block_table.data_ptr<int>(),
                              seq_lens.data_ptr<int>(), bf16p_mut(out), nseq,
                              nq, nkv, hd, q.stride(0), W, bs, (int)max_qlen,
                              (float)scale, fp8 ? 1 : 0,
                              scaled ? k_scale->data_ptr<float>() : nullptr,
                              scaled ? v_scale->data_ptr<float>() : nullptr,
                              (int)window, stream());
    check_launch("attn_prefill_paged");
    return out;
}

Tensor grouped_gemm(const Tensor& x, const Tensor& w, const Tensor& offs) {
    check_bf16(x, "x");
    check_bf16(w, "w");
    TORCH_CHECK(offs.scalar_type() == torch::kInt32 && offs.is_contiguous());
    TORCH_CHECK(x.is_contiguous() && w.is_contiguous());
    const int S = x.size(0), K = x.size(1);
    const int E = w.size(0), N = w.size(1);
    TORCH_CHECK(w.size(2) == K, "K mismatch");
    TORCH_CHECK(offs.size(0) == E + 1);
    TORCH_CHECK(N % 64 == 0, "N must be a multiple of 64");
    TORCH_CHECK(K % 128 == 0, "K must be a multiple of 128");
    Tensor out = torch::empty({S, N}, x.options());
    if (S > 0 && E > 0 && N > 0) {
        launch_grouped_gemm(bf16p(x), bf16p(w), offs.data_ptr<int>(),
                            bf16p_mut(out), E, S, N, K, stream());
        check_launch("grouped_gemm");
    }
    return out;
}

// Seeded per-row sampling (sample.hip): logits [B, V] bf16 | fp32 with any
// row stride -> int64 [B]. Every per-row parameter is a device tensor, so
// nothing here reads a value; top_k and seen_slot values out of range are
// clamped by the kernel.
Tensor sample_rows(const Tensor& logits, const Tensor& temperature,
                   const Tensor& top_k, const Tensor& top_p,
                   const Tensor& penalty, const OptTensor& seen_pool,
                   const Tensor& seen_slot, const Tensor& seed,
                   const Tensor& pos) {
    TORCH_CHECK(logits.is_cuda(), "sample_rows: logits must be on GPU");
    const bool f32 = logits.scalar_type() == torch::kFloat32;
    TORCH_CHECK(f32 || logits.scalar_type() == torch::kBFloat16,
                "sample_rows: logits must be bf16 or fp32");
    TORCH_CHECK(logits.dim() == 2, "sample_rows: logits must be [B, V]");
    const long B = logits.size(0), V = logits.size(1);
    TORCH_CHECK(V >= 1 && V <= INT_MAX && B <= INT_MAX,
                "sample_rows: need 1 <= V and B, V within int32");
    TORCH_CHECK(logits.stride(1) == 1 || V == 1,
                "sample_rows: the last dimension of logits must be "
                "contiguous (any row stride is fine)");
    TORCH_CHECK(B <= 1 || logits.stride(0) >= 0,
                "sample_rows: negative row stride");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) %
                        logits.element_size() == 0,
                "sample_rows: logits are not element-aligned");
    struct Row { const Tensor* t; torch::ScalarType ty; const char* name; };
    const Row rows[] = {{&temperature, torch::kFloat32, "temperature (fp32)"},
                        {&top_k, torch::kInt32, "top_k (int32)"},
                        {&top_p, torch::kFloat32, "top_p (fp32)"},
                        {&penalty, torch::kFloat32, "penalty (fp32)"},
                        {&seen_slot, torch::kInt32, "seen_slot (int32)"},
                        {&seed, torch::kInt64, "seed (int64)"},
                        {&pos, torch::kInt32, "pos (int32)"}};
    for (const Row& r : rows)
        TORCH_CHECK(r.t->is_cuda() && r.t->device() == logits.device() &&
                        r.t->scalar_type() == r.ty && r.t->dim() == 1 &&
                        r.t->size(0) == B && r.t->is_contiguous(),
                    "sample_rows: ", r.name, " must be [B] contiguous on the "
                    "logits' device, B = ", B);
    const unsigned char* pool = nullptr;
    long pool_stride = 0;
    int n_slots = 0;
    if (seen_pool.has_value()) {
        const Tensor& sp = *seen_pool;
        TORCH_CHECK(sp.is_cuda() && sp.device() == logits.device() &&
                        (sp.scalar_type() == torch::kBool ||
                         sp.scalar_type() == torch::kUInt8),
                    "sample_rows: seen_pool must be bool or uint8 on the "
                    "logits' device");
        TORCH_CHECK(sp.dim() == 2 && sp.size(1) == V && sp.size(0) >= 1 &&
                        sp.size(0) <= INT_MAX && sp.is_contiguous(),
                    "sample_rows: seen_pool must be [S, V] contiguous, "
                    "S >= 1, V = ", V);
        pool = static_cast<const unsigned char*>(sp.data_ptr());
        pool_stride = V;
        n_slots = (int)sp.size(0);
    }
    Tensor out = torch::empty({B}, logits.options().dtype(torch::kInt64));
    if (B == 0) return out;
    launch_sample_rows(logits.data_ptr(), f32 ? 1 : 0, logits.stride(0),
                       (int)B, (int)V, temperature.data_ptr<float>(),
                       top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                       penalty.data_ptr<float>(), pool, pool_stride, n_slots,
                       seen_slot.data_ptr<int>(),
                       reinterpret_cast<const long long*>(
                           seed.data_ptr<int64_t>()),
                       pos.data_ptr<int>(),
                       reinterpret_cast<long long*>(out.data_ptr<int64_t>()),
                       stream());
    check_launch("sample_rows");
    return out;
}

Tensor mfma_probe_fp8(const Tensor& A, const Tensor& B) {
    TORCH_CHECK(A.scalar_type() == torch::kUInt8 &&
                B.scalar_type() == torch::kUInt8);
    TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}));
    TORCH_CHECK(B.sizes() == torch::IntArrayRef({32, 16}));
    TORCH_CHECK(A.is_contiguous() && B.is_contiguous());
    Tensor C = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
    launch_mfma_probe_fp8(A.data_ptr<unsigned char>(),
                          B.data_ptr<unsigned char>(), C.data_ptr<float>(),
                          stream());
    check_launch("mfma_probe_fp8");
    return C;
}

Tensor mfma_probe(const Tensor& A, const Tensor& B) {
    check_bf16(A, "A");
    check_bf16(B, "B");
    TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}));
    TORCH_CHECK(B.sizes() == torch::IntArrayRef({32, 16}));
    TORCH_CHECK(A.is_contiguous() && B.is_contiguous());
    Tensor C = torch::empty({16, 16},
                            A.options().dtype(torch::kFloat32));
    launch_mfma_probe(bf16p(A), bf16p(B), C.data_ptr<float>(), stream());
    check_launch("mfma_probe");
    return C;
}

// Pattern probes. mode: 0 linear, 1 row per lane (16 B per lane, the K
// pattern), 2 row per instruction (4 B per lane, the V pattern); + 4 reads
// with non-temporal loads (modes 1 and 2). bw_probe_paged: nt != 0 likewise.
void check_probe_pool(const Tensor& pool, int64_t hd) {
    check_bf16(pool, "pool");
    TORCH_CHECK(pool.is_contiguous() && hd >= 64 && hd % 64 == 0 &&
                    pool.numel() >= hd && pool.numel() % hd == 0,
                "bw_probe: pool must be contiguous, a whole number of rows "
                "of hd elements, hd a multiple of 64");
}

void bw_probe_paged(const Tensor& pool, const Tensor& table, int64_t hd,
                    int64_t rows_per_page, int64_t nt) {
    check_probe_pool(pool, hd);
    const long n_rows = pool.numel() / hd;
    TORCH_CHECK(rows_per_page > 0 && table.is_cuda() &&
                    table.scalar_type() == torch::kInt32 &&
                    table.is_contiguous() &&
                    n_rows % rows_per_page == 0 &&
                    table.numel() * rows_per_page == n_rows,
                "bw_probe_paged: the pool must be whole pages and table "
                "int32 on GPU with one entry (a page index) per page");
    Tensor sink = torch::zeros({1}, pool.options().dtype(torch::kFloat32));
    launch_bw_paged(bf16p(pool), table.data_ptr<int>(), n_rows, (int)hd,
                    (int)rows_per_page, (int)nt, sink.data_ptr<float>(),
                    stream());
    check_launch("bw_probe_paged");
}

void bw_probe(const Tensor& pool, int64_t mode, int64_t hd, int64_t arg) {
    check_probe_pool(pool, hd);
    TORCH_CHECK(mode >= 0 && mode <= 6 && mode != 3 && mode != 4,
                "bw_probe: mode must be 0, 1, 2, 5 (1 + nt) or 6 (2 + nt)");
    Tensor sink = torch::zeros({1}, pool.options().dtype(torch::kFloat32));
    const long n = pool.numel();
    const int nt = (int)(mode >> 2), pat = (int)(mode & 3);
    if (pat == 0)
        launch_bw_linear(bf16p(pool), n, sink.data_ptr<float>(), stream());
    else if (pat == 1)
        launch_bw_rowperlane(bf16p(pool), n / hd, hd, (int)arg, nt,
                             sink.data_ptr<float>(), stream());
    else {
        TORCH_CHECK(arg > 0, "bw_probe: rows per workgroup must be positive");
        launch_bw_rowperinstr(bf16p(pool), n / hd, hd, (int)arg, nt,
                              sink.data_ptr<float>(), stream());
    }
    check_launch("bw_probe");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("rmsnorm", &rmsnorm, "fused RMSNorm (bf16)");
    m.def("fused_add_rmsnorm", &fused_add_rmsnorm,
          "residual += x; y = rmsnorm(residual)");
    m.def("rope_inplace", &rope_inplace, "llama RoPE in place");
    m.def("qk_norm_rope_inplace", &qk_norm_rope_inplace,
          "per-head q/k RMSNorm + RoPE in place (Qwen3)");
    namespace py = pybind11;
    m.def("kv_cache_store", &kv_cache_store, "paged KV scatter",
          py::arg("k"), py::arg("v"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("slots"), py::arg("k_inv_scale") = py::none(),
          py::arg("v_inv_scale") = py::none());
    m.def("rope_kv_store", &rope_kv_store,
          "rope_inplace then kv_cache_store, one kernel where it can",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("pos"),
          py::arg("cos"), py::arg("sin"), py::arg("k_cache"),
          py::arg("v_cache"), py::arg("slots"),
          py::arg("k_inv_scale") = py::none(),
          py::arg("v_inv_scale") = py::none());
    m.def("swiglu", &swiglu, "silu(g) * u");
    m.def("layernorm", &layernorm, "LayerNorm (bf16, weight+bias)");
    m.def("fused_add_layernorm", &fused_add_layernorm,
          "residual add + LayerNorm");
    m.def("gelu", &gelu, "gelu_new (tanh approximation)");
    m.def("attn_decode", &attn_decode, "paged GQA decode attention",
          py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_table"), py::arg("seq_lens"), py::arg("scale"),
          py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none(),
          py::arg("window") = 0);
    m.def("attn_decode_lse", &attn_decode_lse,
          "paged GQA decode attention + per-head (m, l) merge state",
          py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_table"), py::arg("seq_lens"), py::arg("scale"),
          py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none(),
          py::arg("window") = 0);
    m.def("attn_decode_select", &attn_decode_select,
          "attn_decode_lse with an explicit kernel path and Z cap",
          py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
          py::arg("block_table"), py::arg("seq_lens"), py::arg("scale"),
          py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none(),
          py::arg("window") = 0, py::arg("path") = 0, py::arg("max_z") = 0);
    m.def("attn_prefill", &attn_prefill, "varlen causal flash prefill",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("cu_seqlens"),
          py::arg("max_seqlen"), py::arg("scale"), py::arg("causal"),
          py::arg("window") = 0);
    m.def("attn_prefill_paged", &attn_prefill_paged,
          "chunked prefill vs paged history", py::arg("q"),
          py::arg("k_cache"), py::arg("v_cache"), py::arg("block_table"),
          py::arg("seq_lens"), py::arg("cu_q"), py::arg("max_qlen"),
          py::arg("scale"), py::arg("k_scale") = py::none(),
          py::arg("v_scale") = py::none(), py::arg("window") = 0);
    m.def("sample_rows", &sample_rows,
          "seeded per-row temperature / top-k / top-p / penalty sampling",
          py::arg("logits"), py::arg("temperature"), py::arg("top_k"),
          py::arg("top_p"), py::arg("penalty"), py::arg("seen_pool"),
          py::arg("seen_slot"), py::arg("seed"), py::arg("pos"));
    m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA layout probe");
    m.def("mfma_probe_fp8", &mfma_probe_fp8,
          "16x16x32 fp8 MFMA layout probe");
    m.def("grouped_gemm", &grouped_gemm, "per-expert segment GEMM (MoE)");
    m.def("bw_probe", &bw_probe, "bandwidth pattern probe");
    m.def("bw_probe_paged", &bw_probe_paged, "paged row-per-lane probe",
          py::arg("pool"), py::arg("table"), py::arg("hd"),
          py::arg("rows_per_page"), py::arg("nt") = 0);
}
