"""Shared "outlier" input of the per-head fp8 KV scale tests (CPU and GPU).

Four kv heads whose K/V magnitudes span five orders of magnitude: head 0
overflows e4m3's +-448 under a unit scale, head 1 sits in its subnormals,
heads 2 and 3 have unit magnitude. q is divided by the head's K std so the
logits stay O(1) in every head.
"""
import torch

NKV = 4
BS = 32
K_STD = (40.0, 0.01, 1.0, 1.0)
V_STD = (900.0, 0.004, 1.0, 1.0)
E4M3_MAX = 448.0


def _std(vals, *shape):
    return torch.tensor(vals, dtype=torch.float32).view(*shape)


def outlier_kv(n_tokens, hd, gen, dtype=torch.float32):
    """K, V [n_tokens, NKV, hd] with the per-head stds above."""
    k = torch.randn(n_tokens, NKV, hd, generator=gen) * _std(K_STD, 1, NKV, 1)
    v = torch.randn(n_tokens, NKV, hd, generator=gen) * _std(V_STD, 1, NKV, 1)
    return k.to(dtype), v.to(dtype)


def outlier_q(n_rows, G, hd, gen, dtype=torch.float32):
    """q [n_rows, NKV * G, hd] ~ 0.3 * randn / (that head's K std)."""
    q = 0.3 * torch.randn(n_rows, NKV, G, hd, generator=gen)
    q = q / _std(K_STD, 1, NKV, 1, 1)
    return q.reshape(n_rows, NKV * G, hd).to(dtype)


def amax_scales(k, v):
    """(k_scale, v_scale) fp32 [NKV] = per-head amax / 448 of the actual
    K/V, plus their reciprocals (computed once, like PagedKV does)."""
    ks = k.float().abs().amax(dim=(0, 2)) / E4M3_MAX
    vs = v.float().abs().amax(dim=(0, 2)) / E4M3_MAX
    return ks, vs, 1.0 / ks, 1.0 / vs


def permuted_block_table(B, W, gen):
    """[B, W] int32 table over blocks 1..B*W in random order (block 0 is
    never used). Returns (table, n_blocks)."""
    nb = B * W + 1
    perm = torch.randperm(nb - 1, generator=gen) + 1
    return perm[: B * W].reshape(B, W).to(torch.int32), nb


def per_head(x, G):
    """[rows, NKV * G, hd] -> [NKV, rows * G * hd] (one row per kv head)."""
    rows, _nq, hd = x.shape
    return x.float().reshape(rows, NKV, G * hd).permute(1, 0, 2).reshape(NKV, -1)


def rel_l2_per_head(got, truth, G):
    g, t = per_head(got, G), per_head(truth, G)
    return (g - t).norm(dim=1) / t.norm(dim=1)


def div_by_v_std(x, G):
    """Bring every kv head's rows of an attention output to unit magnitude
    (outputs differ by orders of magnitude between heads)."""
    rows, nq, hd = x.shape
    return (x.float().reshape(rows, NKV, G, hd)
            / _std(V_STD, 1, NKV, 1, 1).to(x.device)).reshape(rows, nq, hd)
