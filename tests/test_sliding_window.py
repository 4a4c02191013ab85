"""Sliding-window attention (Mistral-family), CPU side: the reference ops
against a brute-force band mask, logits against transformers' Mistral, config
parsing, KV page release, and the engine end to end.

Semantics: window w > 0, a query at absolute position i attends keys j with
i - w < j <= i; window 0 is off."""
import dataclasses
import json
import os
import threading

import pytest
import torch

from bee2bee_amd.engine.kv import PagedKV
from bee2bee_amd.engine.runner import Runner
from bee2bee_amd.models.spec import PRESETS, ModelSpec, resolve_spec
from bee2bee_amd.models.weights import ModelWeights, save_hf
from bee2bee_amd.ops import reference as R

CPU = torch.device("cpu")
BS = 16


def small_spec(sliding_window, max_seq_len=512, name="sw-tiny"):
    return ModelSpec(
        name=name, vocab_size=128, hidden_size=64, intermediate_size=128,
        n_layers=2, n_heads=4, n_kv_heads=2, head_dim=16, rope_theta=10000.0,
        max_seq_len=max_seq_len, sliding_window=sliding_window,
    )


# ------------------------------------------------ 1. reference ops vs brute

def _dense_attn(q, keys, vals, mask, scale):
    """q [Q, nq, hd], keys/vals [L, nkv, hd], mask [Q, L] True = attend.
    Returns out [Q, nq, hd] and per-(row, head) scores masked to -inf."""
    nq, nkv = q.shape[1], keys.shape[1]
    k = keys.repeat_interleave(nq // nkv, dim=1)
    v = vals.repeat_interleave(nq // nkv, dim=1)
    s = torch.einsum("qhd,lhd->hql", q, k) * scale
    s = s.masked_fill(~mask.unsqueeze(0), float("-inf"))
    out = torch.einsum("hql,lhd->qhd", torch.softmax(s, dim=-1), v)
    return out, s


def _paged(lens, nkv, hd, seed, stale_below=None):
    """fp32 paged cache with a shuffled block table; returns the dense
    per-sequence K/V too. stale_below[b]: table entries of pages wholly
    below that key are pointed at an out-of-range page, so an op that
    indexes them raises."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    W = (max(lens) + BS - 1) // BS
    nb = B * W + 1
    kc = torch.randn(nb, nkv, BS, hd, generator=g)
    vc = torch.randn(nb, nkv, BS, hd, generator=g)
    bt = (torch.randperm(nb - 1, generator=g)[: B * W] + 1).reshape(B, W)
    bt = bt.to(torch.int32)
    dense = []
    for b, L in enumerate(lens):
        blocks = bt[b, : (L + BS - 1) // BS].long()
        kd = kc[blocks].permute(1, 0, 2, 3).reshape(nkv, -1, hd)[:, :L]
        vd = vc[blocks].permute(1, 0, 2, 3).reshape(nkv, -1, hd)[:, :L]
        dense.append((kd.transpose(0, 1), vd.transpose(0, 1)))
    if stale_below is not None:
        for b, lo in enumerate(stale_below):
            bt[b, : max(lo, 0) // BS] = nb + 1000
    return kc, vc, bt, dense


WINDOWS = [1, 5, 16, 40]
LENS = [1, 3, 16, 17, 39, 40, 41, 75]  # both sides of every window


@pytest.mark.parametrize("window", WINDOWS)
def test_reference_decode_matches_band_mask(window):
    nkv, G, hd = 2, 2, 8
    los = [max(0, L - window) for L in LENS]
    kc, vc, bt, dense = _paged(LENS, nkv, hd, seed=window, stale_below=los)
    q = torch.randn(len(LENS), nkv * G, hd,
                    generator=torch.Generator().manual_seed(9))
    lens = torch.tensor(LENS, dtype=torch.int32)
    scale = hd ** -0.5
    out = R.attn_decode(q, kc, vc, bt, lens, scale, window=window)
    out2, ml = R.attn_decode_lse(q, kc, vc, bt, lens, scale, window=window)
    assert torch.equal(out, out2)
    for b, L in enumerate(LENS):
        j = torch.arange(L)
        mask = ((j > L - 1 - window) & (j <= L - 1)).view(1, L)
        ref, s = _dense_attn(q[b: b + 1], *dense[b], mask, scale)
        assert torch.allclose(out[b], ref[0], atol=1e-5), (window, L)
        m = s[:, 0].amax(-1)                       # over the live keys only
        l = torch.exp(s[:, 0] - m.unsqueeze(-1)).sum(-1)
        assert torch.allclose(ml[b, :, 0], m, atol=1e-5), (window, L)
        assert torch.allclose(ml[b, :, 1], l, atol=1e-5), (window, L)
        assert int(mask.sum()) == min(window, L)


@pytest.mark.parametrize("window", WINDOWS)
def test_reference_prefill_matches_band_mask(window):
    nkv, G, hd = 2, 2, 8
    g = torch.Generator().manual_seed(window)
    T = sum(LENS)
    q = torch.randn(T, nkv * G, hd, generator=g)
    k = torch.randn(T, nkv, hd, generator=g)
    v = torch.randn(T, nkv, hd, generator=g)
    cu = [0]
    for L in LENS:
        cu.append(cu[-1] + L)
    scale = hd ** -0.5
    out = R.attn_prefill(q, k, v, torch.tensor(cu, dtype=torch.int32),
                         max(LENS), scale, True, window=window)
    for b, L in enumerate(LENS):
        i = torch.arange(L).view(L, 1)
        j = torch.arange(L).view(1, L)
        mask = (j > i - window) & (j <= i)
        sl = slice(cu[b], cu[b + 1])
        ref, _ = _dense_attn(q[sl], k[sl], v[sl], mask, scale)
        assert torch.allclose(out[sl], ref, atol=1e-5), (window, L)
    with pytest.raises(ValueError):
        R.attn_prefill(q, k, v, torch.tensor(cu, dtype=torch.int32),
                       max(LENS), scale, False, window=window)


@pytest.mark.parametrize("window", WINDOWS)
def test_reference_history_matches_band_mask(window):
    nkv, G, hd = 2, 2, 8
    hist_q = [(0, 9), (5, 1), (16, 16), (30, 20), (41, 7), (70, 5)]
    lens = [h + ql for h, ql in hist_q]
    los = [max(0, h - window + 1) for h, _ in hist_q]
    kc, vc, bt, dense = _paged(lens, nkv, hd, seed=50 + window,
                               stale_below=los)
    T = sum(ql for _, ql in hist_q)
    q = torch.randn(T, nkv * G, hd,
                    generator=torch.Generator().manual_seed(3))
    scale = hd ** -0.5
    out = R.attn_decode_with_history(
        q, kc, vc, bt, torch.tensor(lens, dtype=torch.int32),
        torch.tensor([ql for _, ql in hist_q], dtype=torch.int32), scale,
        window=window)
    t0 = 0
    for b, (h, ql) in enumerate(hist_q):
        i = (h + torch.arange(ql)).view(ql, 1)
        j = torch.arange(lens[b]).view(1, -1)
        mask = (j > i - window) & (j <= i)
        ref, _ = _dense_attn(q[t0: t0 + ql], *dense[b], mask, scale)
        assert torch.allclose(out[t0: t0 + ql], ref, atol=1e-5), (window, h)
        t0 += ql


def test_reference_window_off_is_exactly_todays_output():
    nkv, G, hd = 2, 2, 8
    kc, vc, bt, _ = _paged(LENS, nkv, hd, seed=1)
    g = torch.Generator().manual_seed(2)
    q = torch.randn(len(LENS), nkv * G, hd, generator=g)
    lens = torch.tensor(LENS, dtype=torch.int32)
    scale = hd ** -0.5
    base, base_ml = R.attn_decode_lse(q, kc, vc, bt, lens, scale)
    assert torch.equal(base, R.attn_decode(q, kc, vc, bt, lens, scale))
    for w in (0, max(LENS), 10 ** 6):
        out, ml = R.attn_decode_lse(q, kc, vc, bt, lens, scale, window=w)
        assert torch.equal(out, base) and torch.equal(ml, base_ml), w

    T = sum(LENS)
    pq = torch.randn(T, nkv * G, hd, generator=g)
    pk = torch.randn(T, nkv, hd, generator=g)
    pv = torch.randn(T, nkv, hd, generator=g)
    cu = torch.tensor([0] + list(torch.tensor(LENS).cumsum(0)),
                      dtype=torch.int32)
    base = R.attn_prefill(pq, pk, pv, cu, max(LENS), scale, True)
    for w in (0, max(LENS), 10 ** 6):
        assert torch.equal(
            R.attn_prefill(pq, pk, pv, cu, max(LENS), scale, True, window=w),
            base), w

    qlens = torch.tensor([1, 2, 5, 9, 20, 1, 30, 40], dtype=torch.int32)
    hq = torch.randn(int(qlens.sum()), nkv * G, hd, generator=g)
    base = R.attn_decode_with_history(hq, kc, vc, bt, lens, qlens, scale)
    for w in (0, max(LENS), 10 ** 6):
        assert torch.equal(
            R.attn_decode_with_history(hq, kc, vc, bt, lens, qlens, scale,
                                       window=w), base), w


# --------------------------------------------- 2. logits vs transformers

def _hf_mistral(path):
    transformers = pytest.importorskip("transformers")
    hf = transformers.MistralForCausalLM.from_pretrained(
        path, torch_dtype=torch.float32, attn_implementation="eager")
    return hf.eval()


def _prefill_logits(spec, w, ids, chunk=None):
    """Logits [T, V] of one sequence through Runner.forward_prefill: the
    whole prompt at once, or in chunks against the paged history."""
    kv = PagedKV(spec, CPU, torch.float32, n_blocks=8, block_size=BS)
    runner = Runner(spec, w, kv, CPU, torch.float32)
    T = len(ids)
    kv.new_seq(0)
    rows = []
    step = chunk or T
    for s in range(0, T, step):
        e = min(T, s + step)
        kv.extend_seq(0, e)
        slots = torch.tensor(kv.slot_mapping(0, range(s, e)),
                             dtype=torch.int32)
        kw = {}
        if chunk:
            kw = dict(block_table=kv.block_table([0]),
                      seq_lens=torch.tensor([e], dtype=torch.int32),
                      query_lens=torch.tensor([e - s], dtype=torch.int32))
        hidden = runner.forward_prefill(
            torch.tensor(ids[s:e]), torch.arange(s, e, dtype=torch.int32),
            slots, torch.tensor([0, e - s], dtype=torch.int32), e - s, **kw)
        rows.append(runner.lm_head(hidden))
    return torch.cat(rows)


@pytest.mark.parametrize("sliding_window", [8, None])
def test_logits_match_transformers_mistral(tmp_path, sliding_window):
    """The test that fails without the window: T=40 against a Mistral
    checkpoint with sliding_window=8 (0.18 max logit difference when the
    engine runs full causal attention)."""
    spec = small_spec(sliding_window)
    w = ModelWeights(spec, CPU, torch.float32).random_init(5)
    save_hf(w, str(tmp_path))
    hf = _hf_mistral(str(tmp_path))
    if sliding_window:
        assert hf.config.sliding_window == sliding_window
    else:  # the Mistral config class fills in its own default: beyond T
        assert (hf.config.sliding_window or 10 ** 9) > 40
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(0, spec.vocab_size, (40,), generator=g).tolist()
    with torch.no_grad():
        hf_logits = hf(torch.tensor([ids])).logits[0]
    spec2 = resolve_spec("x", model_path=str(tmp_path))
    assert spec2.sliding_window == sliding_window
    w2 = ModelWeights(spec2, CPU, torch.float32).load_hf(str(tmp_path))
    for chunk in (None, 7):
        ours = _prefill_logits(spec2, w2, ids, chunk=chunk)
        err = (ours - hf_logits).abs().max().item()
        print(f"sliding_window={sliding_window} chunk={chunk}: "
              f"max logit diff {err:.3e}")
        assert err < 2e-3, (
            f"logits diverge from transformers (chunk={chunk}): {err}")


# ---------------------------------------------------- 3. config parsing

def _cfg_dir(tmp_path, **over):
    cfg = {
        "architectures": ["MistralForCausalLM"], "model_type": "mistral",
        "vocab_size": 32000, "hidden_size": 4096,
        "intermediate_size": 14336, "num_hidden_layers": 32,
        "num_attention_heads": 32, "num_key_value_heads": 8,
        "rms_norm_eps": 1e-5, "rope_theta": 10000.0,
        "max_position_embeddings": 32768, "sliding_window": 4096,
    }
    cfg.update(over)
    cfg = {k: v for k, v in cfg.items() if v != "__absent__"}
    d = tmp_path / f"cfg{len(os.listdir(tmp_path))}"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg))
    return str(d)


def test_config_sliding_window_parsing(tmp_path):
    assert resolve_spec("m", _cfg_dir(tmp_path)).sliding_window == 4096
    assert resolve_spec(
        "m", _cfg_dir(tmp_path, sliding_window=None)).sliding_window is None
    assert resolve_spec(
        "m", _cfg_dir(tmp_path, sliding_window="__absent__")
    ).sliding_window is None
    # every Qwen2.5 checkpoint: a window value behind a false flag
    qwen = dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"],
                num_hidden_layers=28, sliding_window=131072,
                max_window_layers=28)
    assert resolve_spec(
        "q", _cfg_dir(tmp_path, use_sliding_window=False, **qwen)
    ).sliding_window is None
    # per-layer windows are refused, not served wrong
    qwen["max_window_layers"] = 21
    with pytest.raises(ValueError, match="per-layer"):
        resolve_spec("q", _cfg_dir(tmp_path, use_sliding_window=True, **qwen))
    # presets
    assert PRESETS["zephyr-7b"].sliding_window == 4096
    assert resolve_spec("mistralai/Mistral-7B-v0.1").sliding_window == 4096
    assert PRESETS["mixtral-8x7b"].sliding_window is None
    assert PRESETS["llama3-8b"].sliding_window is None


def test_save_hf_round_trips_the_window(tmp_path):
    d_win, d_off = str(tmp_path / "win"), str(tmp_path / "off")
    for d, sw in ((d_win, 24), (d_off, None)):
        spec = small_spec(sw)
        save_hf(ModelWeights(spec, CPU, torch.float32).random_init(1), d)
    assert resolve_spec("x", d_win).sliding_window == 24
    assert resolve_spec("x", d_off).sliding_window is None
    cfg_win = json.load(open(os.path.join(d_win, "config.json")))
    cfg_off = json.load(open(os.path.join(d_off, "config.json")))
    assert cfg_win["sliding_window"] == 24
    assert cfg_win["model_type"] == "mistral"
    assert cfg_win["architectures"] == ["MistralForCausalLM"]
    # a windowless config is what it was before the window existed
    assert list(cfg_off) == [
        "architectures", "vocab_size", "hidden_size", "intermediate_size",
        "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
        "head_dim", "rope_theta", "attention_bias", "rms_norm_eps",
        "max_position_embeddings", "tie_word_embeddings", "bos_token_id",
        "eos_token_id"]
    assert cfg_off["architectures"] == ["LlamaForCausalLM"]


def test_export_mask_is_banded():
    from bee2bee_amd.models.export import ExportableModel

    spec = small_spec(8)
    w = ModelWeights(spec, CPU, torch.float32).random_init(5)
    ids = torch.randint(0, spec.vocab_size, (30,),
                        generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        exp = ExportableModel(spec, w).eval()(ids.unsqueeze(0))[0]
    ours = _prefill_logits(spec, w, ids.tolist())
    assert (exp - ours).abs().max().item() < 2e-3


# ------------------------------------------------- 4. PagedKV.release_below

def test_release_below():
    spec = small_spec(None)
    kv = PagedKV(spec, CPU, torch.float32, n_blocks=10, block_size=BS)
    kv.new_seq(7)
    kv.extend_seq(7, 70)  # 5 pages
    assert kv.free_blocks == 5 and kv.seq_live_blocks(7) == 5
    slots_before = kv.slot_mapping(7, range(40, 70))
    pages = kv.block_table([7])[0].tolist()

    # a boundary inside page 2 keeps the straddling page
    assert kv.release_below(7, 2 * BS + 5) == 2
    assert kv.free_blocks == 7
    assert kv.seq_live_blocks(7) == 3 and kv.seq_n_blocks(7) == 5
    assert kv.seq_len(7) == 70
    assert kv.block_table([7])[0].tolist() == [0, 0] + pages[2:]
    assert kv.slot_mapping(7, range(40, 70)) == slots_before
    # idempotent: nothing is released twice
    assert kv.release_below(7, 2 * BS + 5) == 0
    assert kv.release_below(7, 2 * BS) == 0
    assert kv.release_below(7, -3) == 0
    assert kv.free_blocks == 7
    assert sorted(kv._free) == sorted(set(kv._free))

    # growing after a release keeps the logical layout
    kv.extend_seq(7, 100)  # 7 pages
    assert kv.seq_n_blocks(7) == 7 and kv.seq_live_blocks(7) == 5
    assert kv.release_below(7, 3 * BS) == 1
    assert kv.block_table([7])[0].tolist()[:3] == [0, 0, 0]
    # a second sequence can take the released pages
    kv.new_seq(8)
    kv.extend_seq(8, 6 * BS)
    assert kv.free_blocks == 0
    # far past the end: everything goes, never more than the pages held
    assert kv.release_below(7, 10 ** 6) == 4
    assert kv.seq_live_blocks(7) == 0
    kv.free_seq(7)
    kv.free_seq(8)
    assert kv.free_blocks == 10
    assert sorted(kv._free) == list(range(10))


# ------------------------------------------------------- 5. engine end to end

ENGINE_KW = dict(device="cpu", max_batch=1, max_seq_len=1024,
                 max_prefill_tokens=96, seed=3,
                 # the pool is max_batch * 4 pages of 256 tokens plus this
                 # margin, and the engine's scratch sequence keeps one page:
                 # one margin page is what lets a 900-token request (4
                 # pages) be admitted at all
                 kv_margin_blocks=1)
PROMPT_LEN, NEW = 600, 300


def _run_engine(model_path, watch=None, **kw):
    from bee2bee_amd.engine.engine import GenerationRequest, InferenceEngine
    from bee2bee_amd.engine.sampler import SamplingParams

    spec = resolve_spec("sw", model_path=model_path)
    eng = InferenceEngine(spec, model_path=model_path, **ENGINE_KW, **kw)
    try:
        g = torch.Generator().manual_seed(23)
        prompt = torch.randint(3, spec.vocab_size, (PROMPT_LEN,),
                               generator=g).tolist()
        seen = []
        finished = threading.Event()

        # on_emit runs on the engine thread, after the step's pages were
        # released and (for the last token) before the sequence is freed,
        # so every observation is of a settled state
        def on_emit(_tok, done):
            if watch is not None:
                seen.append(watch(eng))
            if done:
                finished.set()

        req = GenerationRequest(
            prompt_ids=prompt, max_new_tokens=NEW,
            sampling=SamplingParams(greedy=True), on_emit=on_emit)
        eng.submit(req)
        assert finished.wait(timeout=300), "generation did not finish"
        assert req.error is None, req.error
        return eng, prompt, list(req.output_ids), seen
    finally:
        eng.shutdown()


@pytest.fixture(scope="module")
def sw_checkpoint(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sw_ckpt"))
    spec = small_spec(64, max_seq_len=1024)
    save_hf(ModelWeights(spec, CPU, torch.float32).random_init(13), d)
    return d


@pytest.fixture(scope="module")
def sw_run(sw_checkpoint):
    def watch(eng):
        sid = eng._active[0].seq_id if eng._active else None
        live = eng.kv.seq_live_blocks(sid) if sid is not None else None
        return live, eng.kv.free_blocks

    return _run_engine(sw_checkpoint, watch=watch)


def test_engine_window_matches_transformers_teacher_forced(sw_checkpoint,
                                                           sw_run):
    eng, prompt, out, _ = sw_run
    assert eng.sliding_window == 64 and len(out) == NEW
    hf = _hf_mistral(sw_checkpoint)
    assert hf.config.sliding_window == 64
    full = prompt + out
    with torch.no_grad():
        logits = hf(torch.tensor([full])).logits[0]
    # row p predicts token p + 1: the emitted token must be (within 1e-3
    # of) that row's maximum — robust to argmax ties
    rows = logits[PROMPT_LEN - 1: PROMPT_LEN - 1 + NEW]
    picked = rows.gather(1, torch.tensor(out).view(-1, 1)).squeeze(1)
    gap = (rows.amax(-1) - picked)
    print(f"teacher-forced max gap {float(gap.max()):.3e}")
    assert float(gap.max()) < 1e-3, (
        f"{int((gap >= 1e-3).sum())} of {NEW} tokens are not the "
        f"transformers argmax; first at {int((gap >= 1e-3).nonzero()[0])}")


def test_engine_window_releases_pages(sw_run):
    eng, _prompt, _out, seen = sw_run
    lives = [live for live, _ in seen if live is not None]
    assert lives and max(lives) <= 2, max(lives)
    # just before the sequence is freed: the last observation with the
    # sequence still active
    last_free = [free for live, free in seen if live is not None][-1]
    assert last_free >= 2, last_free
    assert eng.kv.free_blocks == eng.kv.n_blocks - 1  # scratch page only


def test_engine_window_zero_releases_nothing(sw_checkpoint):
    def watch(eng):
        sid = eng._active[0].seq_id if eng._active else None
        if sid is None:
            return None
        return eng.kv.seq_n_blocks(sid) - eng.kv.seq_live_blocks(sid)

    eng, _p, out, seen = _run_engine(sw_checkpoint, watch=watch,
                                     sliding_window=0)
    assert eng.sliding_window == 0 and eng.runner.window == 0
    assert len(out) == NEW
    assert [r for r in seen if r] == []


def test_engine_window_spec_decode_is_output_invariant(sw_checkpoint, sw_run):
    _eng, _prompt, out, _ = sw_run
    eng, _p, out_spec, _ = _run_engine(sw_checkpoint, spec_decode=True)
    assert eng.sliding_window == 64
    assert out_spec == out


# ------------------------------------------- 6. refusals and the no-op case

def test_cp_engine_refuses_a_window():
    from bee2bee_amd.parallel.cp import CPEngine, cp_attn_decode

    spec = dataclasses.replace(PRESETS["tiny"], sliding_window=64)
    with pytest.raises(ValueError, match="sliding"):
        CPEngine(spec, device="cpu", max_seq_len=512)
    with pytest.raises(ValueError, match="sliding"):
        cp_attn_decode(None, None, None, None, None, 1.0, window=64)


def test_window_covering_every_context_is_off():
    from bee2bee_amd.engine.engine import InferenceEngine

    spec = dataclasses.replace(PRESETS["tiny"], sliding_window=64)
    for msl, want in ((64, 0), (48, 0), (65, 64)):
        eng = InferenceEngine(spec, device="cpu", max_batch=1,
                              max_seq_len=msl, seed=1)
        try:
            assert eng.sliding_window == want, msl
            assert eng.runner.window == want
            assert eng.stats()["sliding_window"] == want
        finally:
            eng.shutdown()
