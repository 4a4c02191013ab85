"""Sliding-window attention on the GPU: the HIP decode / prefill kernels with
`window > 0` against ops.reference with the same window.

Every cache is built so that reading what the window forbids shows up in the
output instead of passing silently:
  * page 0 is unused and finite (the page padding and released entries
    point to);
  * one POISON page is all NaN, and every block-table entry whose page lies
    wholly below the band (and every entry past L) points at it;
  * in the page that straddles the band's lower edge, the rows below the
    edge carry K * 50, so a row that escaped the mask would own the softmax.
A kernel that reads what it must not gives NaN or a wrong answer; it cannot
fault, because every table entry is a valid page index. The reference never
touches the poison page by construction (asserted: its output is finite).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.ops import reference as R

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load
BS = 32                  # page size of every cache here
ZERO_PAGE, POISON = 0, 1
E4M3_NAN = 0x7F


def assert_close(a, b, atol=2e-2, rtol=2e-2, msg=""):
    a = a.float().cpu()
    b = b.float().cpu()
    assert bool(torch.isfinite(b).all()), f"{msg}: reference is not finite"
    assert bool(torch.isfinite(a).all()), (
        f"{msg}: {int((~torch.isfinite(a)).sum())}/{a.numel()} non-finite "
        "outputs (a masked or released page was read)")
    diff = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = diff > tol
    assert not bool(bad.any()), (
        f"{msg}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; "
        f"max diff {float(diff.max()):.4f}"
    )


class Cache:
    """Paged K/V + block table for sequences with lengths `lens` whose first
    live key is `los[b]` (see the module docstring). Page layout: 0 finite
    and unused, 1 poison, 2..33 the straddling page for each value of
    lo % BS (rows below the edge: K * 50), then the live pages — one per
    (sequence, position), or `shared` pages aliased by every table."""

    def __init__(self, lens, los, nkv, hd, fp8=False, scaled=False,
                 shared=0, kmag=1.0, seed=0):
        g = torch.Generator().manual_seed(seed)
        B = len(lens)
        W = (max(lens) + BS - 1) // BS + 1  # one spare column past L
        n_live = shared or B * W
        first_live = 2 + BS
        nb = first_live + n_live
        ksrc = torch.randn(nb, nkv, BS, hd, generator=g) * kmag
        vsrc = torch.randn(nb, nkv, BS, hd, generator=g) * kmag
        for r in range(1, BS):  # straddling page for lo % BS == r
            ksrc[2 + r, :, :r] *= 50.0
        bt = torch.full((B, W), POISON, dtype=torch.int32)
        live = torch.randperm(n_live, generator=g) + first_live
        for b, (L, lo) in enumerate(zip(lens, los)):
            for p in range(W):
                if (p + 1) * BS <= lo or p * BS >= L:
                    continue  # wholly below the band, or past L: poison
                if p * BS < lo:
                    bt[b, p] = 2 + lo % BS
                elif shared:
                    bt[b, p] = int(live[(b * 7 + p) % n_live])
                else:
                    bt[b, p] = int(live[b * W + p])
        self.bt = bt.to(DEV)
        self.lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
        self.k_scale = self.v_scale = None
        if not fp8:
            self.kc = ksrc.to(DEV).bfloat16()
            self.vc = vsrc.to(DEV).bfloat16()
            self.kc[POISON] = float("nan")
            self.vc[POISON] = float("nan")
            return
        # fp8: quantize through the store kernel, as the engine does
        self.kc = torch.zeros(nb, nkv, BS, hd, dtype=torch.uint8, device=DEV)
        self.vc = torch.zeros_like(self.kc)
        kf = ksrc.permute(0, 2, 1, 3).reshape(nb * BS, nkv, hd)
        vf = vsrc.permute(0, 2, 1, 3).reshape(nb * BS, nkv, hd)
        slots = torch.arange(nb * BS, dtype=torch.int32, device=DEV)
        kw = {}
        if scaled:
            self.k_scale = (torch.rand(nkv, generator=g) * 0.06 + 0.02).to(DEV)
            self.v_scale = (torch.rand(nkv, generator=g) * 0.06 + 0.02).to(DEV)
            kw = {"k_inv_scale": 1.0 / self.k_scale,
                  "v_inv_scale": 1.0 / self.v_scale}
        ops.kv_cache_store(kf.to(DEV).bfloat16(), vf.to(DEV).bfloat16(),
                           self.kc, self.vc, slots, **kw)
        self.kc[POISON] = E4M3_NAN
        self.vc[POISON] = E4M3_NAN

    def scales(self):
        if self.k_scale is None:
            return {}
        return {"k_scale": self.k_scale, "v_scale": self.v_scale}


def decode_cache(lens, window, nkv, hd, **kw):
    return Cache(lens, [max(0, L - window) for L in lens], nkv, hd, **kw)


def check_decode(lens, window, nkv, G, hd, atol=2e-2, lse=False, **kw):
    c = decode_cache(lens, window, nkv, hd, **kw)
    g = torch.Generator().manual_seed(100 + len(lens))
    q = (torch.randn(len(lens), nkv * G, hd, generator=g)
         * (0.2 if kw.get("fp8") else 1.0)).to(DEV).bfloat16()
    scale = hd ** -0.5
    msg = f"decode lens={lens[:4]} w={window} nkv{nkv} G{G} hd{hd} {kw}"
    ref, r_ml = R.attn_decode_lse(q, c.kc, c.vc, c.bt, c.lens, scale,
                                  window=window, **c.scales())
    got = ops.attn_decode(q, c.kc, c.vc, c.bt, c.lens, scale,
                          window=window, **c.scales())
    assert_close(got, ref, atol=atol, rtol=atol, msg=msg)
    if lse:
        out, ml = ops.attn_decode_lse(q, c.kc, c.vc, c.bt, c.lens, scale,
                                      window=window, **c.scales())
        assert_close(out, got, msg=msg + " lse out == plain out")
        # the bounds of test_attn_decode_lse_merge, (m, l) over live keys
        assert bool(torch.isfinite(ml).all()), msg
        assert torch.allclose(ml[..., 0], r_ml[..., 0], atol=0.25,
                              rtol=0.02), \
            (ml[..., 0] - r_ml[..., 0]).abs().max()
        assert torch.allclose(ml[..., 1] / r_ml[..., 1].clamp_min(1e-6),
                              torch.ones_like(r_ml[..., 1]), atol=0.1), \
            "sum-exp mismatch"


DECODE_SHAPES = [
    (8, 4, 128),   # llama3-8b / mistral-7b
    (4, 7, 128),   # qwen2.5-7b group
    (8, 4, 64),    # mfma hd 64
    (2, 2, 16),    # generic scores kernel
    (1, 1, 128),
]


@pytest.mark.parametrize("nkv,G,hd", DECODE_SHAPES)
@pytest.mark.parametrize(
    "lens,window",
    [
        # mid-chunk straddle with a skipped chunk; a 1-key last chunk;
        # shorter than the window
        ([500, 257, 40], 128),
        ([512], 256),   # lo exactly on a chunk edge
        ([513], 256),   # one past the chunk edge
        ([300, 33, 1], 1),  # single live key
    ],
)
def test_decode_window(lens, window, nkv, G, hd):
    check_decode(lens, window, nkv, G, hd)


@pytest.mark.parametrize("scaled", [False, True])
def test_decode_window_fp8(scaled):
    check_decode([500, 257, 40], 128, 8, 4, 128, atol=3e-2, fp8=True,
                 scaled=scaled, kmag=0.7)


def test_decode_window_fold_path():
    """B*nkv >= 4096 makes the launcher fold the chunk merge into the PV
    kernel; 520..700 keys are 3 chunks, of which a 128-key window skips one
    or two. All tables alias one small pool, so the cache stays small."""
    B = 512
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(520, 701, (B,), generator=g).tolist()
    lens[0], lens[1] = 520, 700
    check_decode(lens, 128, 8, 4, 64, shared=40, lse=True)


def test_decode_window_combine_path():
    """Small B*nkv: one workgroup per chunk, early-returning workgroups for
    the chunks past L, and the combine kernel walking c0..nc only."""
    check_decode([2048, 1500], 128, 2, 4, 128, lse=True)
    check_decode([2048, 1500], 600, 2, 4, 128, lse=True)


def _packed_qkv(lens, nq, nkv, hd, seed):
    g = torch.Generator().manual_seed(seed)
    T = sum(lens)
    qkv = (torch.randn(T, (nq + 2 * nkv) * hd, generator=g) * 0.5)
    qkv = qkv.to(DEV).bfloat16()
    q = qkv[:, : nq * hd].view(T, nq, hd)
    k = qkv[:, nq * hd: (nq + nkv) * hd].view(T, nkv, hd)
    v = qkv[:, (nq + nkv) * hd:].view(T, nkv, hd)
    cu = [0]
    for ln in lens:
        cu.append(cu[-1] + ln)
    return q, k, v, torch.tensor(cu, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize(
    "lens,window,nq,nkv,hd",
    [
        # rows of the second q tile see a fully masked first key tile
        # before their first live key (the p = 0 guard at m_run = -1e30)
        ([128], 16, 32, 8, 128),
        ([70, 200], 64, 32, 8, 128),
        ([65], 64, 4, 4, 128),
        ([10, 300, 1], 64, 32, 8, 64),
        ([33, 50], 8, 4, 2, 16),   # basic fallback
    ],
)
def test_prefill_window(lens, window, nq, nkv, hd):
    q, k, v, cu = _packed_qkv(lens, nq, nkv, hd, seed=7)
    scale = hd ** -0.5
    got = ops.attn_prefill(q, k, v, cu, max(lens), scale, True,
                           window=window)
    ref = R.attn_prefill(q, k, v, cu, max(lens), scale, True, window=window)
    assert_close(got, ref, atol=3e-2, rtol=3e-2,
                 msg=f"prefill {lens} w={window} hd{hd}")


def check_prefill_paged(hist_q, window, nq, nkv, hd, **kw):
    lens = [h + ql for h, ql in hist_q]
    los = [max(0, h - window + 1) for h, _ in hist_q]
    c = Cache(lens, los, nkv, hd, kmag=0.5, seed=11, **kw)
    g = torch.Generator().manual_seed(12)
    T = sum(ql for _, ql in hist_q)
    q = (torch.randn(T, nq, hd, generator=g) * 0.5).to(DEV).bfloat16()
    cu = [0]
    for _, ql in hist_q:
        cu.append(cu[-1] + ql)
    cu = torch.tensor(cu, dtype=torch.int32, device=DEV)
    qlens = torch.tensor([ql for _, ql in hist_q], dtype=torch.int32,
                         device=DEV)
    scale = hd ** -0.5
    got = ops.attn_prefill_paged(q, c.kc, c.vc, c.bt, c.lens, cu,
                                 max(ql for _, ql in hist_q), scale,
                                 window=window, **c.scales())
    ref = R.attn_decode_with_history(q, c.kc, c.vc, c.bt, c.lens, qlens,
                                     scale, window=window, **c.scales())
    assert_close(got, ref, atol=3e-2, rtol=3e-2,
                 msg=f"prefill_paged {hist_q} w={window} hd{hd} {kw}")


@pytest.mark.parametrize(
    "hist_q,window,nq,nkv,hd",
    [
        ([(200, 70), (0, 64), (300, 1)], 96, 32, 8, 128),
        ([(128, 64)], 96, 32, 8, 64),
        ([(130, 20), (0, 10)], 24, 4, 2, 16),   # basic fallback
    ],
)
def test_prefill_paged_window(hist_q, window, nq, nkv, hd):
    check_prefill_paged(hist_q, window, nq, nkv, hd)


@pytest.mark.parametrize("scaled", [False, True])
def test_prefill_paged_window_fp8(scaled):
    check_prefill_paged([(200, 70), (0, 64)], 96, 32, 8, 128, fp8=True,
                        scaled=scaled)


def test_window_off_is_bit_identical():
    """window=0 and a window that covers the whole context give exactly the
    output of the call without the argument."""
    nkv, G, hd = 8, 4, 128
    lens = [500, 257, 40]
    c = decode_cache(lens, 10 ** 6, nkv, hd)  # nothing below the band
    q = torch.randn(len(lens), nkv * G, hd, device=DEV).bfloat16()
    scale = hd ** -0.5
    base = ops.attn_decode(q, c.kc, c.vc, c.bt, c.lens, scale)
    for w in (0, 500, 4096):
        got = ops.attn_decode(q, c.kc, c.vc, c.bt, c.lens, scale, window=w)
        assert torch.equal(got, base), f"decode window={w}"
    b_out, b_ml = ops.attn_decode_lse(q, c.kc, c.vc, c.bt, c.lens, scale)
    for w in (0, 500):
        out, ml = ops.attn_decode_lse(q, c.kc, c.vc, c.bt, c.lens, scale,
                                      window=w)
        assert torch.equal(out, b_out) and torch.equal(ml, b_ml), w

    plens = [70, 200]
    pq, pk, pv, cu = _packed_qkv(plens, 32, 8, 128, seed=3)
    base = ops.attn_prefill(pq, pk, pv, cu, max(plens), scale, True)
    for w in (0, 200, 4096):
        got = ops.attn_prefill(pq, pk, pv, cu, max(plens), scale, True,
                               window=w)
        assert torch.equal(got, base), f"prefill window={w}"

    hist_q = [(200, 70), (0, 64)]
    plens = [h + ql for h, ql in hist_q]
    pc = Cache(plens, [0, 0], nkv, hd, kmag=0.5)
    T = sum(ql for _, ql in hist_q)
    q2 = (torch.randn(T, nkv * G, hd, device=DEV) * 0.5).bfloat16()
    cu2 = torch.tensor([0, 70, 134], dtype=torch.int32, device=DEV)
    base = ops.attn_prefill_paged(q2, pc.kc, pc.vc, pc.bt, pc.lens, cu2, 70,
                                  scale)
    for w in (0, 270, 4096):
        got = ops.attn_prefill_paged(q2, pc.kc, pc.vc, pc.bt, pc.lens, cu2,
                                     70, scale, window=w)
        assert torch.equal(got, base), f"prefill_paged window={w}"


def test_window_argument_checks():
    q, k, v, cu = _packed_qkv([16], 4, 2, 16, seed=1)
    with pytest.raises(RuntimeError, match="window"):
        ops.attn_prefill(q, k, v, cu, 16, 0.25, False, window=4)
    with pytest.raises(RuntimeError, match="window"):
        ops.attn_prefill(q, k, v, cu, 16, 0.25, True, window=-1)


def test_engine_graphs_see_released_pages():
    """tiny with a 64-key window: the sequence passes 256 + 64 tokens while
    decoding, so its first page is released mid-run. Captured-graph decode
    and eager decode must emit the same greedy ids, which needs the graph's
    block-table copy to pick up the released entry."""
    from bee2bee_amd.engine.engine import InferenceEngine

    prompt = [(i * 37 + 11) % 500 + 3 for i in range(300)]
    outs = {}
    for graphs in (True, False):
        eng = InferenceEngine("tiny", device=DEV, max_batch=2,
                              max_seq_len=512, seed=7, sliding_window=64,
                              kv_margin_blocks=0, use_graphs=graphs)
        try:
            assert (eng.graphs is not None) == graphs
            assert eng.sliding_window == 64
            free0 = eng.kv.free_blocks
            released = []
            release_below = eng.kv.release_below

            def counting(seq_id, first_live_key):
                n = release_below(seq_id, first_live_key)
                if n:
                    released.append((first_live_key, n))
                return n

            eng.kv.release_below = counting
            req = eng.generate(
                prompt, max_new_tokens=40, temperature=0.0,
                repetition_penalty=1.0)
            assert len(req.output_ids) == 40
            outs[graphs] = list(req.output_ids)
            # exactly the first page, once the 256th key left the window,
            # and well before the last decode step
            assert released == [(256, 1)], released
            assert eng.kv.free_blocks == free0
        finally:
            eng.shutdown()
    assert outs[True] == outs[False]
