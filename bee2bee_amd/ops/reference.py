"""Pure-PyTorch fp32 reference implementations of every engine op.

These are the numerics ground truth that the HIP kernels are tested against
(tests/test_ops_gpu.py compares each CDNA4 kernel to these at fp32), and the
CPU execution path for GPU-less environments (plumbing tests, BASELINE
config 1). On a GPU box the engine REQUIRES the HIP extension — see
ops/__init__.py dispatch.

Conventions (shared with the HIP kernels):
  x        [T, H]            activations (T = tokens in batch/chunk)
  q        [T, n_heads, hd]
  k, v     [T, n_kv, hd]
  k_cache  [n_blocks, n_kv, block_size, hd]   paged KV pool
  block_table [B, max_blocks] int32
  slot_mapping [T] int32     flat slot = block_id * block_size + offset
  cos/sin  [max_len, hd/2]   fp32 RoPE tables (host-precomputed)
RoPE is llama-style rotate_half: pair (i, i + hd/2).

Sliding window (`window` keyword of the attention ops, 0 = off): a query at
absolute position i attends keys j with i - window < j <= i, `window` keys
including itself (transformers' Mistral mask). With a window the paged ops
never index a block_table entry whose page lies wholly below the band: the
engine hands such pages back to the pool and their entries go stale.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    norm = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (norm * weight.float()).to(x.dtype)


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    new_residual = (x.float() + residual.float()).to(x.dtype)
    return rmsnorm(new_residual, weight, eps), new_residual


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              eps: float) -> torch.Tensor:
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    out = (xf - mean) * torch.rsqrt(var + eps)
    return (out * weight.float() + bias.float()).to(x.dtype)


def fused_add_layernorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor,
    bias: torch.Tensor, eps: float,
) -> Tuple[torch.Tensor, torch.Tensor]:
    new_residual = (x.float() + residual.float()).to(x.dtype)
    return layernorm(new_residual, weight, bias, eps), new_residual


def gelu(x: torch.Tensor) -> torch.Tensor:
    """HF gelu_new (tanh approximation) — GPT-2's activation."""
    xf = x.float()
    c = 0.7978845608028654 * (xf + 0.044715 * xf.pow(3))
    return (0.5 * xf * (1.0 + torch.tanh(c))).to(x.dtype)


def rope_tables(
    max_len: int, head_dim: int, theta: float, device, dtype=torch.float32,
    scaling: "Optional[dict]" = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host-precomputed cos/sin tables. `scaling` supports the llama3
    rope_type (Llama-3.1/3.2 checkpoints): frequencies below the low-freq
    wavelength divide by `factor`, above high-freq stay, in between
    interpolate smoothly — matches transformers' llama3 rope init."""
    import math

    inv_freq = 1.0 / (
        theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim)
    )
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        factor = float(scaling["factor"])
        lo_f = float(scaling.get("low_freq_factor", 1.0))
        hi_f = float(scaling.get("high_freq_factor", 4.0))
        orig = float(scaling.get("original_max_position_embeddings", 8192))
        low_wl = orig / lo_f
        high_wl = orig / hi_f
        wavelen = 2 * math.pi / inv_freq
        scaled = torch.where(wavelen > low_wl, inv_freq / factor, inv_freq)
        smooth = (orig / wavelen - lo_f) / (hi_f - lo_f)
        mid = (1 - smooth) * inv_freq / factor + smooth * inv_freq
        is_mid = (wavelen <= low_wl) & (wavelen >= high_wl)
        inv_freq = torch.where(is_mid, mid, scaled)
    t = torch.arange(max_len, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)  # [max_len, hd/2]
    return freqs.cos().to(device, dtype), freqs.sin().to(device, dtype)


def rope_inplace(
    q: torch.Tensor,
    k: torch.Tensor,
    positions: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
) -> None:
    hd = q.shape[-1]
    c = cos[positions].unsqueeze(1)  # [T, 1, hd/2]
    s = sin[positions].unsqueeze(1)
    for t in (q, k):
        # .float() is identity for fp32 tensors — clone so the first-half
        # write cannot alias the second-half read
        tf = t.detach().clone().float()
        x1, x2 = tf[..., : hd // 2], tf[..., hd // 2 :]
        t[..., : hd // 2] = (x1 * c - x2 * s).to(t.dtype)
        t[..., hd // 2 :] = (x2 * c + x1 * s).to(t.dtype)


def qk_norm_rope_inplace(
    q: torch.Tensor,
    k: torch.Tensor,
    positions: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    q_weight: torch.Tensor,
    k_weight: torch.Tensor,
    eps: float,
) -> None:
    """Qwen3 attention prologue: RMSNorm of every q head and every k head
    over head_dim (one [hd] weight for all q heads, one for all k heads),
    then rotate-half RoPE. fp32 throughout; the single rounding to the
    tensor dtype is the final write."""
    hd = q.shape[-1]
    pos = positions.long()
    c = cos[pos].unsqueeze(1).float()  # [T, 1, hd/2]
    s = sin[pos].unsqueeze(1).float()
    for t, w in ((q, q_weight), (k, k_weight)):
        xf = t.detach().clone().float()
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        xf = xf * w.float()
        x1, x2 = xf[..., : hd // 2], xf[..., hd // 2 :]
        t[..., : hd // 2] = (x1 * c - x2 * s).to(t.dtype)
        t[..., hd // 2 :] = (x2 * c + x1 * s).to(t.dtype)


def _kv_deq(cache: torch.Tensor) -> torch.Tensor:
    """Dequantize an fp8 (OCP e4m3, uint8 storage) cache to fp32; bf16/fp32
    caches pass through as fp32."""
    if cache.dtype == torch.uint8:
        return cache.view(torch.float8_e4m3fn).float()
    return cache.float()


def _kv_quant_like(x: torch.Tensor, cache: torch.Tensor) -> torch.Tensor:
    if cache.dtype == torch.uint8:
        return x.float().to(torch.float8_e4m3fn).view(torch.uint8)
    return x.to(cache.dtype)


E4M3_MAX = 448.0


def _kv_quant_scaled(x: torch.Tensor, inv_scale: torch.Tensor) -> torch.Tensor:
    """Per-kv-head scaled fp8 quantization, the definition the HIP store
    kernel follows: byte = e4m3_rne(clamp(x * inv_scale[h], -448, 448)) in
    fp32. x [T, n_kv, hd], inv_scale [n_kv]."""
    y = x.float() * inv_scale.float().view(1, -1, 1)
    y = y.clamp(-E4M3_MAX, E4M3_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def _check_scales(cache: torch.Tensor, *scales) -> None:
    for s in scales:
        if s is None:
            continue
        if cache.dtype != torch.uint8:
            raise ValueError("per-head KV scales need an fp8 (uint8) cache")
        if s.dtype != torch.float32 or s.shape != (cache.shape[1],):
            raise ValueError("KV scales must be fp32 [n_kv_heads]")


def _head_scale(x: torch.Tensor, s) -> torch.Tensor:
    """x [n_kv, ...] times the per-kv-head scale s [n_kv] (None: unit)."""
    if s is None:
        return x
    return x * s.float().view(-1, *([1] * (x.dim() - 1)))


def kv_cache_store(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_inv_scale: torch.Tensor = None,
    v_inv_scale: torch.Tensor = None,
) -> None:
    n_blocks, n_kv, block_size, hd = k_cache.shape
    _check_scales(k_cache, k_inv_scale, v_inv_scale)
    blk = torch.div(slot_mapping, block_size, rounding_mode="floor").long()
    off = (slot_mapping % block_size).long()
    k_cache[blk, :, off, :] = (
        _kv_quant_like(k, k_cache) if k_inv_scale is None
        else _kv_quant_scaled(k, k_inv_scale))
    v_cache[blk, :, off, :] = (
        _kv_quant_like(v, v_cache) if v_inv_scale is None
        else _kv_quant_scaled(v, v_inv_scale))


def rope_kv_store(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    positions: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_inv_scale: torch.Tensor = None,
    v_inv_scale: torch.Tensor = None,
) -> None:
    """rope_inplace on (q, k), then kv_cache_store of the rotated k and of
    v: by definition the composition of the two reference ops."""
    rope_inplace(q, k, positions, cos, sin)
    kv_cache_store(k, v, k_cache, v_cache, slot_mapping, k_inv_scale,
                   v_inv_scale)


def attn_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_table: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: float,
    out_ml: torch.Tensor = None,
    k_scale: torch.Tensor = None,
    v_scale: torch.Tensor = None,
    window: int = 0,
) -> torch.Tensor:
    """Paged single-token attention, GQA. q [B, nq, hd] -> out [B, nq, hd].
    When out_ml [B, nq, 2] is given, also writes the flash merge state
    (max scaled score m, sum-exp l) per query head — the cross-rank
    exchange for context parallelism. k_scale / v_scale [n_kv] are the
    per-kv-head dequantization scales of a scaled fp8 cache: the scores
    (and so m, l) are taken on float(byte) * k_scale, the output on
    float(byte) * v_scale. window > 0: the query sits at L-1 and only keys
    [max(0, L - window), L) are live; (m, l) are taken over those."""
    B, nq, hd = q.shape
    _nb, n_kv, block_size, _ = k_cache.shape
    _check_scales(k_cache, k_scale, v_scale)
    if window < 0:
        raise ValueError("window must be >= 0 (0 = off)")
    group = nq // n_kv
    out = torch.empty_like(q)
    for b in range(B):
        L = int(seq_lens[b])
        if L == 0:
            # empty context (a CP rank owning no pages of this sequence):
            # zero output with (m, l) = (-inf, 0) merge state
            out[b] = 0
            if out_ml is not None:
                out_ml[b, :, 0] = -1e30
                out_ml[b, :, 1] = 0.0
            continue
        nblk = (L + block_size - 1) // block_size
        # first live key and the page that holds it (0, 0 without a window)
        lo = max(0, L - window) if window > 0 else 0
        b0 = lo // block_size
        blocks = block_table[b, b0:nblk].long()
        keys = _kv_deq(k_cache[blocks])  # [nblk - b0, n_kv, bs, hd]
        vals = _kv_deq(v_cache[blocks])
        span = slice(lo - b0 * block_size, L - b0 * block_size)
        keys = keys.permute(1, 0, 2, 3).reshape(
            n_kv, (nblk - b0) * block_size, hd)[:, span]
        vals = vals.permute(1, 0, 2, 3).reshape(
            n_kv, (nblk - b0) * block_size, hd)[:, span]
        qb = q[b].float().view(n_kv, group, hd)
        scores = torch.einsum("kgd,kld->kgl", qb, keys) * scale
        scores = _head_scale(scores, k_scale)
        probs = torch.softmax(scores, dim=-1)
        ob = _head_scale(torch.einsum("kgl,kld->kgd", probs, vals), v_scale)
        out[b] = ob.reshape(nq, hd).to(q.dtype)
        if out_ml is not None:
            m = scores.amax(dim=-1)                         # [n_kv, group]
            l = torch.exp(scores - m.unsqueeze(-1)).sum(-1)  # [n_kv, group]
            out_ml[b, :, 0] = m.reshape(nq)
            out_ml[b, :, 1] = l.reshape(nq)
    return out


def attn_prefill(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,
    max_seqlen: int,
    scale: float,
    causal: bool = True,
    window: int = 0,
) -> torch.Tensor:
    """Varlen full-prompt attention, GQA. q [T, nq, hd] -> [T, nq, hd].
    window > 0 (causal only): row i attends keys (i - window, i]."""
    T, nq, hd = q.shape
    if window < 0 or (window > 0 and not causal):
        raise ValueError("a sliding window needs window > 0 and causal=True")
    n_kv = k.shape[1]
    group = nq // n_kv
    out = torch.empty_like(q)
    for i in range(cu_seqlens.numel() - 1):
        s, e = int(cu_seqlens[i]), int(cu_seqlens[i + 1])
        L = e - s
        qi = q[s:e].float().view(L, n_kv, group, hd)
        ki = k[s:e].float()
        vi = v[s:e].float()
        scores = torch.einsum("qkgd,lkd->kgql", qi, ki) * scale
        if causal:
            mask = torch.triu(
                torch.ones(L, L, dtype=torch.bool, device=q.device), diagonal=1
            )
            scores.masked_fill_(mask, float("-inf"))
            if window > 0:
                pos = torch.arange(L, device=q.device)
                below = pos.view(1, L) <= pos.view(L, 1) - window
                scores.masked_fill_(below, float("-inf"))
        probs = torch.softmax(scores, dim=-1)
        oi = torch.einsum("kgql,lkd->qkgd", probs, vi)
        out[s:e] = oi.reshape(L, nq, hd).to(q.dtype)
    return out


def attn_decode_with_history(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_table: torch.Tensor,
    seq_lens: torch.Tensor,
    query_lens: torch.Tensor,
    scale: float,
    k_scale: torch.Tensor = None,
    v_scale: torch.Tensor = None,
    window: int = 0,
) -> torch.Tensor:
    """Chunked-prefill attention: multiple new query tokens per sequence
    attending to the full paged history (new tokens already stored in cache).

    q [T, nq, hd] packed by sequence; seq_lens = total length incl. the new
    chunk; query_lens = chunk length per sequence. window > 0: chunk row r
    sits at hist + r (hist = L - QL) and attends keys (hist + r - window,
    hist + r]."""
    if window < 0:
        raise ValueError("window must be >= 0 (0 = off)")
    T, nq, hd = q.shape
    _nb, n_kv, block_size, _ = k_cache.shape
    group = nq // n_kv
    _check_scales(k_cache, k_scale, v_scale)
    out = torch.empty_like(q)
    t0 = 0
    for b in range(query_lens.numel()):
        QL = int(query_lens[b])
        L = int(seq_lens[b])
        nblk = (L + block_size - 1) // block_size
        # the chunk's first row has the lowest band edge: pages wholly
        # below it are not indexed (k0 = first key position gathered)
        lo = max(0, L - QL - window + 1) if window > 0 else 0
        b0 = lo // block_size
        k0 = b0 * block_size
        blocks = block_table[b, b0:nblk].long()
        keys = (
            _kv_deq(k_cache[blocks])
            .permute(1, 0, 2, 3)
            .reshape(n_kv, (nblk - b0) * block_size, hd)[:, : L - k0]
        )
        vals = (
            _kv_deq(v_cache[blocks])
            .permute(1, 0, 2, 3)
            .reshape(n_kv, (nblk - b0) * block_size, hd)[:, : L - k0]
        )
        qb = q[t0 : t0 + QL].float().view(QL, n_kv, group, hd)
        scores = torch.einsum("qkgd,kld->kgql", qb, keys) * scale
        scores = _head_scale(scores, k_scale)
        # causal within the chunk: query j (absolute pos L-QL+j) sees keys <= pos
        qpos = torch.arange(L - QL, L, device=q.device).view(1, 1, QL, 1)
        kpos = torch.arange(k0, L, device=q.device).view(1, 1, 1, L - k0)
        scores.masked_fill_(kpos > qpos, float("-inf"))
        if window > 0:
            scores.masked_fill_(kpos <= qpos - window, float("-inf"))
        probs = torch.softmax(scores, dim=-1)
        ob = torch.einsum("kgql,kld->kgqd", probs, vals)
        ob = _head_scale(ob, v_scale).permute(2, 0, 1, 3)
        out[t0 : t0 + QL] = ob.reshape(QL, nq, hd).to(q.dtype)
        t0 += QL
    return out


def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    g, u = gate_up.float().chunk(2, dim=-1)
    return (torch.nn.functional.silu(g) * u).to(gate_up.dtype)


def moe_topk_gate(
    logits: torch.Tensor, top_k: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Softmax-after-topk gating (Mixtral). logits [T, E] ->
    (weights [T, k] fp32, indices [T, k] int32)."""
    vals, idx = torch.topk(logits.float(), top_k, dim=-1)
    weights = torch.softmax(vals, dim=-1)
    return weights, idx.to(torch.int32)


def grouped_gemm(
    x: torch.Tensor,        # [S, K] (rows sorted by expert)
    w: torch.Tensor,        # [E, N, K]
    offsets: torch.Tensor,  # [E+1] int32
) -> torch.Tensor:
    """Per-expert segment GEMM: out[offs[e]:offs[e+1]] = x_seg @ w[e].T"""
    S, K = x.shape
    E, N, _ = w.shape
    out = torch.zeros(S, N, dtype=x.dtype, device=x.device)
    for e in range(E):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        if hi > lo:
            out[lo:hi] = (x[lo:hi].float() @ w[e].float().t()).to(x.dtype)
    return out


def attn_decode_lse(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_table: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: float,
    k_scale: torch.Tensor = None,
    v_scale: torch.Tensor = None,
    window: int = 0,
):
    """attn_decode + per-head (m, l) merge state (see parallel/cp.py)."""
    out_ml = torch.empty(q.shape[0], q.shape[1], 2, dtype=torch.float32,
                         device=q.device)
    out = attn_decode(q, k_cache, v_cache, block_table, seq_lens, scale,
                      out_ml=out_ml, k_scale=k_scale, v_scale=v_scale,
                      window=window)
    return out, out_ml


# ------------------------------------------------------------------ sampling

SAMPLE_MAX_K = 1024  # candidates the sampler keeps at most (kernel LDS sort)

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def _mulhilo32(a: int, b: torch.Tensor):
    """(hi, lo) words of the 64-bit product a * b; b holds u32 values in
    int64, and no intermediate leaves int64."""
    lo16 = a * (b & 0xFFFF)
    t = a * (b >> 16) + (lo16 >> 16)
    return t >> 16, ((t & 0xFFFF) << 16) | (lo16 & 0xFFFF)


def philox4x32(counter, key, rounds: int = 10) -> torch.Tensor:
    """Philox4x32 (Salmon et al., SC'11). counter [..., 4] and key [..., 2]
    hold u32 words as int64; returns the four output words [..., 4]."""
    c = [torch.as_tensor(counter, dtype=torch.int64)[..., i] & _U32
         for i in range(4)]
    k = [torch.as_tensor(key, dtype=torch.int64)[..., i] & _U32
         for i in range(2)]
    for r in range(rounds):
        if r:
            k = [(k[0] + _PHILOX_W0) & _U32, (k[1] + _PHILOX_W1) & _U32]
        hi0, lo0 = _mulhilo32(_PHILOX_M0, c[0])
        hi1, lo1 = _mulhilo32(_PHILOX_M1, c[2])
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
    return torch.stack(c, dim=-1)


def sample_uniform(seed: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """The sampler's draw u in (0, 1] for (seed int64, pos int32), fp32:
    word 0 of Philox4x32-10 under key (seed_lo, seed_hi) and counter
    (pos, 0, 0, 0), as ((r0 >> 8) + 0.5) * 2^-24 in fp32 arithmetic."""
    seed = seed.to(torch.int64)
    key = torch.stack([seed & _U32, (seed >> 32) & _U32], dim=-1)
    p = pos.to(torch.int64) & _U32
    zero = torch.zeros_like(p)
    r0 = philox4x32(torch.stack([p, zero, zero, zero], dim=-1), key)[..., 0]
    return ((r0 >> 8).to(torch.float32) + 0.5) * (2.0 ** -24)


def sample_sort_key(z: torch.Tensor) -> torch.Tensor:
    """Order-preserving u32 key of fp32 z (as int64): larger z, larger key;
    -0.0 counts as +0.0 and every NaN maps to key 0, below -inf."""
    z = z + 0.0
    bits = z.contiguous().view(torch.int32).to(torch.int64) & _U32
    key = torch.where(bits >= 0x80000000, ~bits & _U32, bits | 0x80000000)
    return torch.where(torch.isnan(z), torch.zeros_like(key), key)


def sample_z(logits, temperature, penalty, seen_pool, seen_slot):
    """Steps 1 and 2 of sample_rows: the penalized, temperature-scaled
    logits z, fp32 [B, V]."""
    x = logits.float()
    if seen_pool is not None:
        slot = seen_slot.to(torch.int64)
        seen = seen_pool[slot.clamp_min(0)].bool() & (slot >= 0)[:, None]
        p = penalty.float()[:, None]
        x = torch.where(seen, torch.where(x > 0, x / p, x * p), x)
    t = temperature.float()
    t = torch.where(t > 1e-5, t, torch.full_like(t, 1e-5))
    return x / t[:, None] + 0.0


def sample_rows(
    logits: torch.Tensor,
    temperature: torch.Tensor,
    top_k: torch.Tensor,
    top_p: torch.Tensor,
    penalty: torch.Tensor,
    seen_pool: Optional[torch.Tensor],
    seen_slot: torch.Tensor,
    seed: torch.Tensor,
    pos: torch.Tensor,
) -> torch.Tensor:
    """Seeded per-row sampling: logits [B, V] bf16 | fp32 -> int64 [B].

    Every row has its own temperature f32, top_k i32, top_p f32, penalty
    f32, seen_slot i32 (row of seen_pool bool/uint8 [S, V]; -1 = none),
    seed i64 and pos i32. Per row:

      1. x = float(logit); a token whose seen bit is set becomes x / penalty
         if x > 0, else x * penalty.
      2. z = x / max(T, 1e-5), in fp32.
      3. The candidates are the k = clamp(top_k, 1, min(V, 1024)) largest
         under the total order (z descending, index ascending).
      4. w_j = exp(z_j - z_0) over the candidates in that order.
      5. With 0 < top_p < 1, candidate j stays while
         (cum_j - w_j) / Z <= top_p (the token that crosses top_p stays).
      6. u = sample_uniform(seed, pos); the result is the first kept j with
         cum_j > u * Z_kept, or the last kept one.

    Greedy is top_k = 1, temperature = 1: the argmax, lowest index on a tie.
    Non-finite values: -0.0 orders as +0.0 and NaN orders below -inf
    (sample_sort_key); a NaN candidate has weight 0; and when the first
    candidate is not finite (+inf, or a row without a finite entry) it is
    the result, so such a row gives its lowest-index +inf, else token 0.
    A NaN temperature reads as 1e-5 and a NaN top_p as off."""
    B, V = logits.shape
    dev = logits.device
    z = sample_z(logits, temperature, penalty, seen_pool, seen_slot)
    kmax = min(V, SAMPLE_MAX_K)
    k = top_k.to(torch.int64).clamp(1, kmax)
    order = torch.sort(sample_sort_key(z), dim=1, descending=True,
                       stable=True).indices[:, :kmax]
    zc = z.gather(1, order)
    j = torch.arange(kmax, device=dev)[None, :]
    valid = j < k[:, None]
    z0 = zc[:, :1]
    w = torch.where(valid & ~torch.isnan(zc), torch.exp(zc - z0),
                    torch.zeros_like(zc))
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    cum = torch.cumsum(w, dim=1, dtype=torch.float32)
    Z = cum.gather(1, (k - 1)[:, None])
    p = top_p.float()[:, None]
    keep = valid & (~((p > 0) & (p < 1)) | ((cum - w) / Z <= p))
    n_kept = keep.to(torch.int64).cumprod(dim=1).sum(dim=1).clamp_min(1)
    thr = sample_uniform(seed, pos).to(dev)[:, None] * cum.gather(
        1, (n_kept - 1)[:, None])
    hit = (cum > thr) & (j < n_kept[:, None])
    first = torch.where(hit, j, torch.full_like(j, kmax)).amin(dim=1)
    choice = torch.minimum(first, n_kept - 1)
    choice = torch.where(torch.isfinite(z0[:, 0]), choice,
                         torch.zeros_like(choice))
    return order.gather(1, choice[:, None])[:, 0]
