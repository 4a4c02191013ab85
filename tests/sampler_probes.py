"""Probe inputs for the sampler tests: cases in which ONE element, one tie,
one boundary or one parameter decides the sampled token, an exact float64
evaluator with a worked-out tolerance for random rows, and mutants (wrong
samplers in plain torch) that prove the cases can tell right from wrong.

Every case is a function case(fn, device, dtype): `fn` has the signature of
ops.reference.sample_rows, and the case asserts on what it returns.
tests/test_sampler_probes.py (CPU) runs every case through the reference,
which must pass, and through every mutant, which must fail a case;
tests/test_sampler_probes_gpu.py runs the same cases through the HIP kernel.

Plain helper module: imports torch and bee2bee_amd.ops.reference only.
"""
import functools
import math

import torch

from bee2bee_amd.ops import reference as R

# the kernel walks a row as a scalar head up to the first 16-byte boundary,
# 16-byte vectors strided over 1024 threads, and a scalar tail
VEC_BYTES = 16
THREADS = 1024


def params(B, device, T=1.0, k=1, p=1.0, pen=1.0, slot=-1, seed=0, pos=0):
    """Per-row parameter tensors from scalars or per-row lists, in the
    order sample_rows takes them (without logits and the pool)."""
    def col(v, dtype):
        if isinstance(v, torch.Tensor):
            return v.to(device=device, dtype=dtype)
        if isinstance(v, (list, tuple)):
            return torch.tensor(v, dtype=dtype, device=device)
        return torch.full((B,), v, dtype=dtype, device=device)
    return dict(temperature=col(T, torch.float32), top_k=col(k, torch.int32),
                top_p=col(p, torch.float32), penalty=col(pen, torch.float32),
                seen_slot=col(slot, torch.int32), seed=col(seed, torch.int64),
                pos=col(pos, torch.int32))


def run(fn, logits, pool=None, **kw):
    q = params(logits.shape[0], logits.device, **kw)
    out = fn(logits, q["temperature"], q["top_k"], q["top_p"], q["penalty"],
             pool, q["seen_slot"], q["seed"], q["pos"])
    assert out.dtype == torch.int64 and out.shape == (logits.shape[0],)
    out = out.cpu()
    assert bool(((out >= 0) & (out < logits.shape[1])).all()), \
        "token outside [0, V)"
    return out


def strided_rows(B, V, device, dtype, fill=0.0):
    """[B, V] rows inside a wider buffer whose row stride is odd, so the
    rows' base addresses take every element offset within 16 bytes."""
    stride = V + (3 if V % 2 == 0 else 4)
    base = torch.full((B, stride), fill, dtype=dtype, device=device)
    x = base[:, 1:1 + V]
    assert x.stride(0) == stride and not x.is_contiguous()
    return x


def row_head(x, r):
    """Elements of row r before its first 16-byte boundary."""
    addr = x.data_ptr() + r * x.stride(0) * x.element_size()
    return min(x.shape[1], ((-addr) % VEC_BYTES) // x.element_size())


def row_edges(x, r):
    """Indices either side of every edge the kernel has in row r: the row
    ends, head | body, a vector, a tile (the thread stride), body | tail."""
    V = x.shape[1]
    n = VEC_BYTES // x.element_size()
    h = row_head(x, r)
    tail0 = h + (V - h) // n * n
    tile = n * THREADS
    cand = {0, 1, V - 2, V - 1, h - 1, h, h + n - 1, h + n, tail0 - 1, tail0}
    for m in range(1, (V - h) // tile + 1):
        cand |= {h + m * tile - 1, h + m * tile}
    return sorted(i for i in cand if 0 <= i < V)


# ------------------------------------------------------- float64 evaluator

def accept_sets(logits, pool=None, tol_terms=4.0, inclusive_top_p=False,
                **kw):
    """Per row, the set of tokens a correct fp32 sampler may return: a
    float64 evaluation of sample_rows' steps on the fp32 z, accepting
    either resolution of a boundary comparison (top-p membership, or the
    inverse-CDF crossing) that lies within tol = tol_terms * k * 2^-24 of
    equality, relative to Z. That is the fp32 bound for a k-term sum in any
    order plus expf. tol_terms = 0 gives the one exact answer."""
    logits = logits.cpu()
    pool = None if pool is None else pool.cpu()
    q = params(logits.shape[0], "cpu", **kw)
    z = R.sample_z(logits, q["temperature"], q["penalty"], pool,
                   q["seen_slot"])
    u = R.sample_uniform(q["seed"], q["pos"]).double()
    B, V = z.shape
    order = torch.sort(R.sample_sort_key(z), dim=1, descending=True,
                       stable=True).indices
    out = []
    for r in range(B):
        k = int(q["top_k"][r].clamp(1, min(V, R.SAMPLE_MAX_K)))
        idx = order[r, :k]
        zc = z[r, idx].double()
        if not math.isfinite(float(zc[0])):
            out.append({int(idx[0])})
            continue
        w = torch.where(torch.isnan(zc), torch.zeros_like(zc),
                        torch.exp(zc - zc[0]))
        cum = torch.cumsum(w, 0)
        Z = float(cum[-1])
        tol = tol_terms * k * 2.0 ** -24
        p = float(q["top_p"][r])
        n_lo = n_hi = k
        if 0.0 < p < 1.0:
            e = (cum if inclusive_top_p else cum - w) / Z
            n_lo = max(1, int((e <= p - tol).sum()))
            n_hi = max(1, int((e <= p + tol).sum()))
        acc = set()
        for n in range(n_lo, n_hi + 1):
            target = float(u[r]) * float(cum[n - 1])
            c = cum[:n]
            ja = min(n - 1, int(torch.searchsorted(
                c, torch.tensor(target - tol * Z, dtype=c.dtype), right=True)))
            jb = min(n - 1, int(torch.searchsorted(
                c, torch.tensor(target + tol * Z, dtype=c.dtype), right=True)))
            acc.update(int(i) for i in idx[ja:jb + 1])
        out.append(acc)
    return out


# -------------------------------------------------------------------- cases

def case_philox(fn, device, dtype):
    """The three known answers of Philox4x32-10."""
    def words(c, k):
        return ["%08x" % v for v in R.philox4x32(
            torch.tensor(c), torch.tensor(k)).tolist()]
    assert words([0] * 4, [0] * 2) == [
        "6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert words([0xffffffff] * 4, [0xffffffff] * 2) == [
        "408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert words([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344],
                 [0xa4093822, 0x299f31d0]) == [
        "d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # the draw built from word 0: (r0 >> 8) + 0.5 scaled by 2^-24, in fp32
    u = R.sample_uniform(torch.tensor([0]), torch.tensor([0]))
    assert float(u) == (0x6627e8 + 0.5) * 2.0 ** -24


def _one_hot(V, fn, device, dtype):
    # the row stride is odd, so the rows' base offsets go round with this
    # period; row r probes edge number r // period of its own edge list,
    # and 32 seeds go round
    period = VEC_BYTES // torch.empty(0, dtype=dtype).element_size()
    n_edges = 10 + 2 * (V // (period * THREADS))
    x = strided_rows(period * n_edges, V, device, dtype)
    heads, want = set(), []
    for r in range(x.shape[0]):
        edges = row_edges(x, r)
        assert len(edges) <= n_edges
        heads.add(row_head(x, r))
        want.append(edges[(r // period) % len(edges)])
        x[r, want[-1]] = 30.0
    assert heads == set(range(period)), heads
    got = run(fn, x, T=1.0, k=64, p=0.95,
              seed=[r % 32 for r in range(x.shape[0])], pos=7)
    assert got.tolist() == want, [
        (r, w, g) for r, (w, g) in enumerate(zip(want, got.tolist()))
        if w != g][:8]


def case_one_hot_512(fn, device, dtype):
    _one_hot(512, fn, device, dtype)


def case_one_hot_4099(fn, device, dtype):
    _one_hot(4099, fn, device, dtype)


def case_one_hot_50257(fn, device, dtype):
    _one_hot(50257, fn, device, dtype)


def _tie_row(V, k, i, j, pair, dtype, device):
    """Equal logits `pair` at i < j, k - 1 tokens at -30 spread over the
    row, everything else at -60."""
    x = torch.full((V,), -60.0)
    others = [t for t in range(0, V, max(1, V // (k + 8)))
              if t not in (i, j)][:k - 1]
    assert len(others) == k - 1
    x[others] = -30.0
    x[i] = x[j] = pair
    return x.to(device=device, dtype=dtype)


def case_tie(fn, device, dtype):
    """A tie goes to the lower index. With the pair on top and top_p 0.4
    only the first candidate stays, so the token is always i; with the
    pair between the -30 tokens and the floor it sits exactly at the k-th
    place, and j is never a candidate."""
    V, seeds = 4099, 32
    for k in (2, 64, 1024):
        i, j = 1033, 3077
        row = _tie_row(V, k, i, j, 0.0, dtype, device)
        x = strided_rows(seeds, V, device, dtype)
        x[:] = row
        got = run(fn, x, T=1.0, k=k, p=0.4, seed=list(range(seeds)), pos=k)
        assert got.tolist() == [i] * seeds, (k, got.tolist())
        # the k-th place: k - 1 tokens at -30, the pair at -30.5
        row = _tie_row(V, k, i, j, -30.5, dtype, device)
        x[:] = row
        got = run(fn, x, T=1.0, k=k, p=1.0, seed=list(range(seeds)), pos=k)
        assert j not in got.tolist(), (k, got.tolist())
        if k == 2:
            assert i in got.tolist(), got.tolist()


def case_top_p_edge(fn, device, dtype):
    """Probabilities (0.5, 0.3, 0.2), top_p 0.6: the token that crosses
    top_p stays, the one after it never appears."""
    seeds = 64
    x = torch.tensor([0.5, 0.3, 0.2]).log().to(device=device, dtype=dtype)
    x = x.repeat(seeds, 1)
    got = run(fn, x, T=1.0, k=3, p=0.6, seed=list(range(seeds)),
              pos=1).tolist()
    assert 2 not in got, got
    assert 1 in got and 0 in got, got


def case_penalty(fn, device, dtype):
    V = 10
    row = torch.zeros(V)
    row[5], row[3] = 2.0, 1.9          # tests/test_sampler.py's landscape
    neg = torch.full((V,), -5.0)
    neg[0], neg[1] = -1.0, -1.2
    pool = torch.zeros(3, V, dtype=torch.bool)
    pool[0, 5] = True                  # slot 0 has seen token 5
    pool[1, 3] = True                  # slot 1 has seen token 3
    pool[2, 0] = True                  # slot 2 has seen token 0
    pool = pool.to(device)
    x = torch.stack([row, row, row, row, neg, neg]).to(device=device,
                                                       dtype=dtype)
    got = run(fn, x, pool=pool, T=1.0, k=1,
              pen=[1.15, 1.15, 1.15, 1.15, 1.5, 1.5],
              slot=[0, -1, 1, 0, 2, -1]).tolist()
    # 2.0 / 1.15 < 1.9; slot -1 untouched; slot 1 leaves 2.0 on top;
    # a negative logit is multiplied: -1.0 * 1.5 < -1.2
    assert got == [3, 5, 5, 3, 1, 0], got
    # two rows with their slots swapped
    got = run(fn, x[:2], pool=pool, T=1.0, k=1, pen=1.15,
              slot=[1, 0]).tolist()
    assert got == [5, 3], got
    # a uint8 pool reads the same
    got = run(fn, x[:2], pool=pool.to(torch.uint8), T=1.0, k=1, pen=1.15,
              slot=[0, 1]).tolist()
    assert got == [3, 5], got


# six parameter sets (T, k, p, penalty, slot), greedy among them
_PARAM_SETS = [
    (1.0, 1, 1.0, 1.0, -1),          # greedy
    (0.7, 64, 0.95, 1.15, 0),
    (1.0, 256, 0.9, 1.0, -1),
    (1.3, 8, 1.0, 1.3, 1),
    (0.5, 1024, 0.5, 1.0, -1),
    (1.0, 1, 1.0, 2.0, 2),           # greedy with a penalty
]


@functools.lru_cache(maxsize=None)
def _mixed_inputs():
    g = torch.Generator().manual_seed(101)
    B, V = 16, 4099
    x = (torch.randn(B, V, generator=g) * 3.0).bfloat16().float()
    pool = torch.rand(3, V, generator=g) < 0.3
    sets = [_PARAM_SETS[r % len(_PARAM_SETS)] for r in range(B)]
    kw = dict(T=[s[0] for s in sets], k=[s[1] for s in sets],
              p=[s[2] for s in sets], pen=[s[3] for s in sets],
              slot=[s[4] for s in sets], seed=[1000 + 7 * r for r in range(B)],
              pos=[r % 5 for r in range(B)])
    return x, pool, kw


def case_per_row(fn, device, dtype):
    """Every row of a 16-row batch with 6 parameter sets equals the same
    row run alone, and the same row at another batch index."""
    x, pool, kw = _mixed_inputs()
    B = x.shape[0]
    x = x.to(device=device, dtype=dtype)
    pool = pool.to(device)
    full = run(fn, x, pool=pool, **kw).tolist()
    # the sampled rows are not all the argmax: the parameters matter
    greedy = run(fn, x, T=1.0, k=1).tolist()
    assert sum(a != b for a, b in zip(full, greedy)) >= 4, (full, greedy)
    for r in range(B):
        one = {key: [v[r]] for key, v in kw.items()}
        assert run(fn, x[r:r + 1], pool=pool, **one).tolist() == [full[r]], r
    perm = [(r + 5) % B for r in range(B)]          # new row n = old perm[n]
    shuffled = {key: [v[i] for i in perm] for key, v in kw.items()}
    got = run(fn, x[torch.tensor(perm, device=x.device)], pool=pool,
              **shuffled).tolist()
    assert got == [full[i] for i in perm]


def case_non_finite(fn, device, dtype):
    """NaN orders below -inf and never wins; a row whose first candidate
    is not finite returns it: the lowest-index +inf, else token 0."""
    V = 515
    nan, inf = float("nan"), float("inf")
    x = torch.zeros(6, V)
    x[0, 0] = nan
    x[0, 400] = 3.0                      # greedy: the finite maximum
    x[1, 7] = x[1, 3] = inf              # lowest-index +inf
    x[2, :] = -inf                       # no finite entry: token 0
    x[3, :] = nan                        # all NaN: token 0
    x[4, :] = nan
    x[4, 9] = -inf                       # -inf orders above NaN
    x[5, :] = -inf
    x[5, 300] = -1e30                    # one finite entry
    x = x.to(device=device, dtype=dtype)
    got = run(fn, x, T=1.0, k=1).tolist()
    assert got == [400, 3, 0, 0, 9, 300], got
    got = run(fn, x, T=0.7, k=64, p=0.9, seed=5, pos=2).tolist()
    assert got[1:] == [3, 0, 0, 9, 300] and got[0] != 0, got
    # sampling over the whole row: -inf and NaN entries carry no weight
    seeds = 64
    y = torch.zeros(seeds, 8)
    y[:, 1] = -inf
    y[:, 6] = nan
    y = y.to(device=device, dtype=dtype)
    got = run(fn, y, T=1.0, k=8, p=1.0, seed=list(range(seeds))).tolist()
    assert 1 not in got and 6 not in got, got
    assert len(set(got)) >= 4, got


# chi-square critical values at the 1 - 1e-6 quantile, df = 1..15
_CHI2_1E6 = [23.928, 27.631, 30.665, 33.377, 35.888, 38.258, 40.522, 42.701,
             44.811, 46.863, 48.866, 50.825, 52.747, 54.635, 56.493]


def case_distribution(fn, device, dtype):
    """20 000 draws (seeds 0..19999, one call) against the exact truncated
    distribution of V = 16, k = 8, p = 0.9: chi-square at the 1e-6
    quantile. The seeds are fixed, so the outcome is fixed."""
    N, V, k, p, T = 20000, 16, 8, 0.9, 0.8
    row = torch.tensor([0.5, -1.25, 2.0, 0.25, 1.5, -0.5, 1.0, 0.0,
                        1.75, -2.0, 0.75, 1.25, -0.75, 2.25, -1.5, 0.125])
    z = row.double() / float(torch.tensor(T, dtype=torch.float32))
    order = torch.argsort(z, descending=True, stable=True)[:k]
    w = torch.exp(z[order] - z[order[0]])
    cum = torch.cumsum(w, 0)
    n_kept = int((((cum - w) / cum[-1]) <= float(
        torch.tensor(p, dtype=torch.float32))).sum())
    prob = w[:n_kept] / cum[n_kept - 1]
    assert 3 <= n_kept < k and float(prob.min()) * N > 100
    x = row.to(device=device, dtype=dtype).repeat(N, 1)
    got = run(fn, x, T=T, k=k, p=p, seed=list(range(N)), pos=3)
    counts = torch.bincount(got, minlength=V).double()
    kept = order[:n_kept]
    assert int(counts.sum() - counts[kept].sum()) == 0, \
        "a token outside the kept set was sampled"
    chi2 = float((((counts[kept] - N * prob) ** 2) / (N * prob)).sum())
    assert chi2 < _CHI2_1E6[n_kept - 2], (chi2, counts[kept].tolist())


RANDOM_SHAPES = {           # name: (V, k, scale, T, p)
    "random_4096_k64": (4096, 64, 3.0, 0.7, 0.95),
    "random_4096_k256": (4096, 256, 3.0, 1.0, 0.9),
    "random_8192_k1024": (8192, 1024, 4.0, 0.7, 0.95),
}
RANDOM_ROWS = 256
MAX_AMBIGUOUS = 0.05     # share of a case's rows that may accept > 1 token


@functools.lru_cache(maxsize=None)
def random_inputs(V, k, scale, T, p, rows=RANDOM_ROWS, seed=2024):
    """bf16-rounded randn * scale rows with their acceptance sets; computed
    once and shared (the reference alone decides what is accepted)."""
    g = torch.Generator().manual_seed(seed + V + k)
    x = (torch.randn(rows, V, generator=g) * scale).bfloat16()
    kw = dict(T=T, k=k, p=p, seed=[31 * r + 5 for r in range(rows)],
              pos=[r % 97 for r in range(rows)])
    acc = accept_sets(x, **kw)
    many = sum(len(a) > 1 for a in acc)
    assert many <= MAX_AMBIGUOUS * rows, (
        f"{many} of {rows} rows accept more than one token")
    return x, kw, acc


def check_accepted(got, acc, what):
    bad = [(r, t, sorted(a)) for r, (t, a) in
           enumerate(zip(got.tolist(), acc)) if t not in a]
    assert not bad, f"{what}: {len(bad)} rows outside the accepted set, " \
                    f"first {bad[:4]}"


def _random(name, fn, device, dtype):
    x, kw, acc = random_inputs(*RANDOM_SHAPES[name])
    got = run(fn, x.to(device=device, dtype=dtype), **kw)
    check_accepted(got, acc, name)


CASES = {
    "philox": case_philox,
    "one_hot_512": case_one_hot_512,
    "one_hot_4099": case_one_hot_4099,
    "one_hot_50257": case_one_hot_50257,
    "tie": case_tie,
    "top_p_edge": case_top_p_edge,
    "penalty": case_penalty,
    "per_row": case_per_row,
    "non_finite": case_non_finite,
    "distribution": case_distribution,
}
for _name in RANDOM_SHAPES:
    CASES[_name] = functools.partial(_random, _name)


# ------------------------------------------------------------------ mutants
# Wrong samplers: the reference behind one deliberate mistake each.

def _ref(x, t, k, p, pen, pool, slot, seed, pos):
    return R.sample_rows(x, t, k, p, pen, pool, slot, seed, pos)


def m_drop_last(x, *a):
    x = x.clone()
    x[:, -1] = -float("inf")
    return _ref(x, *a)


def m_drop_tile_first(x, *a):
    """The first element of every tile after the first is never read."""
    y = x.clone()
    tile = VEC_BYTES // x.element_size() * THREADS
    for r in range(x.shape[0]):
        h = row_head(x, r)
        y[r, h + tile::tile] = -float("inf")
    return _ref(y, *a)


def m_tie_high(x, t, k, p, pen, pool, slot, seed, pos):
    V = x.shape[1]
    pool = None if pool is None else pool.flip(1)
    return V - 1 - _ref(x.flip(1), t, k, p, pen, pool, slot, seed, pos)


def m_k_plus_one(x, t, k, *a):
    return _ref(x, t, k + 1, *a)


def m_top_p_inclusive(x, t, k, p, pen, pool, slot, seed, pos):
    """`cum > top_p` drops a token instead of `cum - w > top_p`."""
    acc = accept_sets(x, pool=pool, tol_terms=0.0, inclusive_top_p=True,
                      T=t, k=k, p=p, pen=pen, slot=slot, seed=seed, pos=pos)
    return torch.tensor([next(iter(a)) for a in acc], dtype=torch.int64)


def m_penalty_divides(x, t, k, p, pen, pool, slot, seed, pos):
    """Seen logits are divided by the penalty whatever their sign."""
    if pool is None:
        return _ref(x, t, k, p, pen, pool, slot, seed, pos)
    s = slot.to(torch.int64)
    seen = pool[s.clamp_min(0)].bool() & (s >= 0)[:, None]
    x = torch.where(seen, x.float() / pen.float()[:, None], x.float())
    return _ref(x, t, k, p, pen, None, slot, seed, pos)


def m_neighbour_slot(x, t, k, p, pen, pool, slot, seed, pos):
    if pool is not None:
        slot = torch.where(slot >= 0, (slot + 1) % pool.shape[0], slot)
    return _ref(x, t, k, p, pen, pool, slot, seed, pos)


def m_u_by_row(x, t, k, p, pen, pool, slot, seed, pos):
    row = torch.arange(x.shape[0], dtype=torch.int64)
    return _ref(x, t, k, p, pen, pool, slot, row, torch.zeros_like(pos))


def m_no_temperature(x, t, *a):
    return _ref(x, torch.ones_like(t), *a)


def m_params_row0(x, t, k, p, pen, pool, slot, seed, pos):
    t, k, p, pen = (v[:1].expand_as(v) for v in (t, k, p, pen))
    return _ref(x, t, k, p, pen, pool, slot, seed, pos)


# mutant -> the cases expected to catch it (at least one must)
MUTANTS = {
    "drop_last": (m_drop_last, ("one_hot_512",)),
    "drop_tile_first": (m_drop_tile_first, ("one_hot_50257",)),
    "tie_high": (m_tie_high, ("tie",)),
    "k_plus_one": (m_k_plus_one, ("tie",)),
    "top_p_inclusive": (m_top_p_inclusive, ("top_p_edge",)),
    "penalty_divides": (m_penalty_divides, ("penalty",)),
    "neighbour_slot": (m_neighbour_slot, ("penalty",)),
    "u_by_row": (m_u_by_row, ("per_row",)),
    "no_temperature": (m_no_temperature, ("distribution",
                                          "random_4096_k64")),
    "params_row0": (m_params_row0, ("per_row",)),
}
