"""Qwen3 family: per-head QK-norm fused with RoPE, a head_dim decoupled
from hidden_size / n_heads, and the Qwen3-MoE config and weight names.

Ground-truth anchors: reference.qk_norm_rope_inplace against a plain-torch
formula, and a checkpoint saved by this framework loaded into transformers'
Qwen3ForCausalLM / Qwen3MoeForCausalLM giving the Runner's logits."""
import json
import os

import pytest
import torch

from bee2bee_amd import ops
from bee2bee_amd.models.spec import PRESETS, resolve_spec, spec_from_hf_config
from bee2bee_amd.models.weights import ModelWeights, save_hf
from bee2bee_amd.ops import reference as R

CPU = torch.device("cpu")


def _weights(name, seed):
    return ModelWeights(PRESETS[name], CPU, torch.float32).random_init(seed)


# ------------------------------------------------------------- reference


def _plain_qk_norm_rope(x, pos, cos, sin, w, eps):
    """Per-head RMSNorm over head_dim, then rotate-half RoPE."""
    var = (x * x).sum(-1, keepdim=True) / x.shape[-1]
    n = x / torch.sqrt(var + eps) * w
    c = torch.cat([cos[pos.long()], cos[pos.long()]], -1)[:, None, :]
    s = torch.cat([sin[pos.long()], sin[pos.long()]], -1)[:, None, :]
    half = x.shape[-1] // 2
    rot = torch.cat([-n[..., half:], n[..., :half]], -1)
    return n * c + rot * s


@pytest.mark.parametrize("nq,nkv,hd", [(4, 2, 16), (3, 1, 64), (2, 1, 128)])
def test_reference_matches_plain_formula(nq, nkv, hd):
    torch.manual_seed(0)
    T, eps = 7, 1e-6
    # strided q/k views of one fused qkv tensor, as the runner passes them
    qkv = torch.randn(T, (nq + 2 * nkv) * hd)
    # per-head magnitudes differ ~100x: a norm taken across heads fails
    qkv.view(T, nq + 2 * nkv, hd).mul_(
        torch.logspace(-1, 1, nq + 2 * nkv)[None, :, None])
    before = qkv.clone()
    qw, kw = 1 + 0.3 * torch.randn(hd), 1 + 0.3 * torch.randn(hd)
    cos, sin = R.rope_tables(64, hd, 10000.0, CPU)
    pos = torch.tensor([5, 0, 63, 2, 2, 40, 1], dtype=torch.int32)
    q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    q, k = q.view(T, nq, hd), k.view(T, nkv, hd)
    want_q = _plain_qk_norm_rope(q.clone(), pos, cos, sin, qw, eps)
    want_k = _plain_qk_norm_rope(k.clone(), pos, cos, sin, kw, eps)
    R.qk_norm_rope_inplace(q, k, pos, cos, sin, qw, kw, eps)
    assert torch.allclose(q, want_q, atol=1e-5, rtol=1e-5)
    assert torch.allclose(k, want_k, atol=1e-5, rtol=1e-5)
    assert torch.equal(v, before[:, (nq + nkv) * hd:])  # v untouched
    # the q and k weights are not interchangeable
    assert not torch.allclose(
        k, _plain_qk_norm_rope(before[:, nq * hd:(nq + nkv) * hd].view(
            T, nkv, hd), pos, cos, sin, qw, eps), atol=1e-3)


def test_ops_dispatch_uses_reference_on_cpu():
    torch.manual_seed(1)
    T, nq, nkv, hd = 3, 2, 1, 16
    q, k = torch.randn(T, nq, hd), torch.randn(T, nkv, hd)
    q2, k2 = q.clone(), k.clone()
    qw, kw = torch.rand(hd) + 0.5, torch.rand(hd) + 0.5
    cos, sin = R.rope_tables(8, hd, 10000.0, CPU)
    pos = torch.tensor([0, 7, 3], dtype=torch.int32)
    ops.qk_norm_rope_inplace(q, k, pos, cos, sin, qw, kw, 1e-6)
    R.qk_norm_rope_inplace(q2, k2, pos, cos, sin, qw, kw, 1e-6)
    assert torch.equal(q, q2) and torch.equal(k, k2)


# ----------------------------------------------------------------- specs


def test_presets_and_aliases():
    t = PRESETS["tiny-qwen3"]
    assert t.qk_norm and t.q_size == 128 and t.hidden_size == 64
    assert PRESETS["tiny-qwen3-moe"].qk_norm
    assert PRESETS["tiny-qwen3-moe"].n_experts == PRESETS["tiny-moe"].n_experts
    s = resolve_spec("Qwen/Qwen3-8B")
    assert (s.name, s.hidden_size, s.intermediate_size, s.n_layers, s.n_heads,
            s.n_kv_heads, s.head_dim, s.tie_embeddings) == (
        "qwen3-8b", 4096, 12288, 36, 32, 8, 128, False)
    assert s.qk_norm and not s.qkv_bias and s.rope_theta == 1e6
    assert s.rms_eps == 1e-6 and s.vocab_size == 151936
    assert resolve_spec("qwen3").name == "qwen3-8b"
    m = resolve_spec("qwen/qwen3-30b-a3b")
    assert (m.n_experts, m.top_k_experts, m.intermediate_size, m.n_layers,
            m.n_heads, m.n_kv_heads) == (128, 8, 768, 48, 32, 4)
    # 0.6B: head_dim 128 with hidden 1024 / 16 heads = 64
    assert PRESETS["qwen3-0.6b"].q_size == 2048


def test_n_params_counts_the_norm_weights():
    import dataclasses

    t = PRESETS["tiny-qwen3"]
    plain = dataclasses.replace(t, qk_norm=False)
    assert t.n_params() - plain.n_params() == t.n_layers * 2 * t.head_dim
    w = _weights("tiny-qwen3", 0)
    counted = w.embed.numel() + w.final_norm.numel()  # tied head
    for lw in w.layers:
        counted += sum(getattr(lw, n).numel() for n in (
            "attn_norm", "mlp_norm", "wqkv", "wo", "w_gate_up", "w_down",
            "q_norm", "k_norm"))
    assert counted == t.n_params()


def test_random_init_norms_are_not_ones():
    w = _weights("tiny-qwen3", 3)
    for lw in w.layers:
        assert lw.q_norm.shape == lw.k_norm.shape == (16,)
        assert (lw.q_norm - 1).abs().max() > 0.05
        assert not torch.equal(lw.q_norm, lw.k_norm)
        assert 0.5 < float(lw.q_norm.mean()) < 1.5
    assert _weights("tiny", 3).layers[0].q_norm is None


# ------------------------------------------------------------ round trip


def test_roundtrip_bit_exact(tmp_path):
    spec = PRESETS["tiny-qwen3"]
    w = _weights("tiny-qwen3", 3)
    save_hf(w, str(tmp_path))
    spec2 = resolve_spec("x", model_path=str(tmp_path))
    assert spec2.qk_norm and spec2.head_dim == 16 and spec2.hidden_size == 64
    assert (spec2.n_heads, spec2.n_kv_heads, spec2.q_size) == (8, 2, 128)
    with open(tmp_path / "config.json") as f:
        cfg = json.load(f)
    assert cfg["model_type"] == "qwen3"
    assert cfg["architectures"] == ["Qwen3ForCausalLM"]
    w2 = ModelWeights(spec2, CPU, torch.float32).load_hf(str(tmp_path))
    assert torch.equal(w.embed, w2.embed)
    assert torch.equal(w.final_norm, w2.final_norm)
    for a, b in zip(w.layers, w2.layers):
        for n in ("attn_norm", "mlp_norm", "wqkv", "wo", "w_gate_up",
                  "w_down", "q_norm", "k_norm"):
            assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert spec.n_layers == len(w2.layers)


def test_layer_range_load_takes_only_its_norms(tmp_path):
    spec = PRESETS["tiny-qwen3"]
    w = _weights("tiny-qwen3", 9)
    save_hf(w, str(tmp_path))
    first = ModelWeights(spec, CPU, torch.float32).load_hf(
        str(tmp_path), layer_range=(0, 1))
    assert torch.equal(first.layers[0].q_norm, w.layers[0].q_norm)
    assert first.layers[1].q_norm is None and first.layers[1].k_norm is None
    last = ModelWeights(spec, CPU, torch.float32).load_hf(
        str(tmp_path), layer_range=(1, 2))
    assert last.layers[0].q_norm is None and last.layers[0].k_norm is None
    assert torch.equal(last.layers[1].k_norm, w.layers[1].k_norm)
    # random_init for a stage draws the same values as the full init
    part = ModelWeights(spec, CPU, torch.float32).random_init(
        9, layer_range=(1, 2))
    assert torch.equal(part.layers[1].q_norm, w.layers[1].q_norm)
    assert part.layers[0].q_norm is None


# ---------------------------------------------------- loader strictness


def _rewrite_tensors(path, fn):
    from safetensors.torch import load_file, save_file

    f = os.path.join(path, "model.safetensors")
    save_file(fn(load_file(f)), f)


def test_missing_q_norm_raises(tmp_path):
    save_hf(_weights("tiny-qwen3", 1), str(tmp_path))
    _rewrite_tensors(str(tmp_path), lambda t: {
        k: v for k, v in t.items()
        if k != "model.layers.1.self_attn.q_norm.weight"})
    spec = resolve_spec("x", model_path=str(tmp_path))
    with pytest.raises(FileNotFoundError, match="q_norm"):
        ModelWeights(spec, CPU, torch.float32).load_hf(str(tmp_path))


def test_llama_config_over_qk_norm_tensors_raises(tmp_path):
    """The hole this closes: a Qwen3 checkpoint parsed as a Llama used to
    load with q_norm / k_norm dropped and serve wrong numerics."""
    save_hf(_weights("tiny-qwen3", 1), str(tmp_path))
    cfg_path = tmp_path / "config.json"
    cfg = json.loads(cfg_path.read_text())
    cfg["model_type"] = "llama"
    cfg["architectures"] = ["LlamaForCausalLM"]
    cfg_path.write_text(json.dumps(cfg))
    spec = resolve_spec("x", model_path=str(tmp_path))
    assert not spec.qk_norm
    with pytest.raises(ValueError, match="q_norm|k_norm"):
        ModelWeights(spec, CPU, torch.float32).load_hf(str(tmp_path))


# ------------------------------------------ equivalence with transformers


def _runner_prefill_logits(spec, w, ids):
    from bee2bee_amd.engine.kv import PagedKV
    from bee2bee_amd.engine.runner import Runner

    kv = PagedKV(spec, CPU, torch.float32, n_blocks=8)
    runner = Runner(spec, w, kv, CPU, torch.float32)
    T = len(ids)
    kv.new_seq(0)
    kv.extend_seq(0, T)
    slots = torch.tensor(kv.slot_mapping(0, range(T)), dtype=torch.int32)
    hidden = runner.forward_prefill(
        torch.tensor(ids), torch.arange(T, dtype=torch.int32), slots,
        torch.tensor([0, T], dtype=torch.int32), T,
    )
    return runner.lm_head(hidden)


IDS = [5, 9, 17, 3, 250, 44, 8]


def test_qwen3_logits_match_transformers(tmp_path):
    """Our runner's prefill logits vs transformers' Qwen3ForCausalLM on the
    SAME saved checkpoint, fp32."""
    transformers = pytest.importorskip("transformers")

    spec = PRESETS["tiny-qwen3"]
    w = _weights("tiny-qwen3", 7)
    save_hf(w, str(tmp_path))
    hf = transformers.Qwen3ForCausalLM.from_pretrained(
        str(tmp_path), torch_dtype=torch.float32)
    hf.eval()
    # the checkpoint's norm weights reached the HF module (not re-initialised)
    assert torch.equal(hf.model.layers[1].self_attn.k_norm.weight.data,
                       w.layers[1].k_norm)
    with torch.no_grad():
        hf_logits = hf(torch.tensor([IDS])).logits[0]  # [T, V]
    ours = _runner_prefill_logits(spec, w, IDS)
    err = (ours - hf_logits).abs().max().item()
    assert err < 2e-3, f"logits diverge from transformers: {err}"


def test_qwen3_moe_logits_match_transformers(tmp_path):
    """Same anchor for the MoE variant: Qwen3MoeForCausalLM loads the
    per-expert mlp.experts.{e}.{gate,up,down}_proj tensors this framework
    writes (checked below: a loaded expert weight equals ours), and the
    logits agree."""
    transformers = pytest.importorskip("transformers")

    spec = PRESETS["tiny-qwen3-moe"]
    w = _weights("tiny-qwen3-moe", 7)
    save_hf(w, str(tmp_path))
    hf = transformers.Qwen3MoeForCausalLM.from_pretrained(
        str(tmp_path), torch_dtype=torch.float32)
    hf.eval()
    sd = hf.state_dict()
    gate = sd["model.layers.1.mlp.gate.weight"]
    assert torch.equal(gate, w.layers[1].moe_gate), "router not loaded"
    fused = [k for k in sd if k.startswith("model.layers.1.mlp.experts.")]
    assert fused, "no expert tensors in the transformers model"
    ours_dn = w.layers[1].moe_w_down  # [E, H, I]
    if "model.layers.1.mlp.experts.down_proj" in sd:
        assert torch.equal(sd["model.layers.1.mlp.experts.down_proj"],
                           ours_dn), "expert weights not loaded"
    else:
        assert torch.equal(
            sd["model.layers.1.mlp.experts.3.down_proj.weight"], ours_dn[3])
    with torch.no_grad():
        hf_logits = hf(torch.tensor([IDS])).logits[0]
    ours = _runner_prefill_logits(spec, w, IDS)
    err = (ours - hf_logits).abs().max().item()
    assert err < 2e-3, f"logits diverge from transformers: {err}"


def test_qwen3_moe_roundtrip_and_expert_range(tmp_path):
    spec = PRESETS["tiny-qwen3-moe"]
    w = _weights("tiny-qwen3-moe", 5)
    save_hf(w, str(tmp_path))
    cfg = json.loads((tmp_path / "config.json").read_text())
    assert cfg["model_type"] == "qwen3_moe"
    assert cfg["num_experts"] == 4 and cfg["moe_intermediate_size"] == 96
    assert cfg["norm_topk_prob"] is True
    spec2 = resolve_spec("x", model_path=str(tmp_path))
    assert (spec2.n_experts, spec2.top_k_experts, spec2.intermediate_size,
            spec2.qk_norm) == (4, 2, 96, True)
    w2 = ModelWeights(spec2, CPU, torch.float32).load_hf(str(tmp_path))
    for a, b in zip(w.layers, w2.layers):
        for n in ("moe_gate", "moe_w_gate_up", "moe_w_down", "q_norm",
                  "k_norm"):
            assert torch.equal(getattr(a, n), getattr(b, n)), n
    shard = ModelWeights(spec2, CPU, torch.float32).load_hf(
        str(tmp_path), expert_range=(2, 4))
    assert shard.layers[0].moe_w_down.shape[0] == 2
    assert torch.equal(shard.layers[0].moe_w_gate_up,
                       w.layers[0].moe_w_gate_up[2:4])
    assert torch.equal(shard.layers[0].moe_gate, w.layers[0].moe_gate)


@pytest.mark.parametrize("patch,what", [
    ({"norm_topk_prob": False}, "norm_topk_prob"),
    ({"mlp_only_layers": [0]}, "mlp_only_layers"),
    ({"decoder_sparse_step": 2}, "decoder_sparse_step"),
])
def test_qwen3_moe_config_rejections(tmp_path, patch, what):
    save_hf(_weights("tiny-qwen3-moe", 5), str(tmp_path))
    cfg_path = tmp_path / "config.json"
    cfg = json.loads(cfg_path.read_text())
    spec_from_hf_config(str(tmp_path))  # as written: accepted
    cfg.update(patch)
    cfg_path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match=what):
        spec_from_hf_config(str(tmp_path))


# ------------------------------------------------------------ engine, CPU

PROMPT = [(i * 7 + 3) % 500 + 4 for i in range(40)]


def _greedy(model="tiny-qwen3", prompt=PROMPT, n=10, **kw):
    from bee2bee_amd.engine.engine import InferenceEngine

    eng = InferenceEngine(model, device="cpu", max_batch=2, max_seq_len=128,
                          seed=11, **kw)
    try:
        assert eng.weights.layers[0].q_norm is not None
        req = eng.generate(prompt, max_new_tokens=n, temperature=0.0,
                           repetition_penalty=1.0)
        assert req.error is None, req.error
        assert len(req.output_ids) == n
        return req.output_ids
    finally:
        eng.shutdown()


@pytest.fixture(scope="module")
def base_tokens():
    return _greedy()


def test_engine_greedy_deterministic(base_tokens):
    assert _greedy() == base_tokens


def test_engine_chunked_prefill_matches_whole(base_tokens):
    assert _greedy(max_prefill_tokens=16) == base_tokens


def test_engine_spec_decode_matches_plain(base_tokens):
    assert _greedy(spec_decode=True) == base_tokens


def test_runner_uses_the_norm_weights(monkeypatch):
    """The runner routes a qk_norm spec through ops.qk_norm_rope_inplace,
    once per layer, with that layer's weights — and the logits depend on
    them (forcing them to ones moves the logits)."""
    spec = PRESETS["tiny-qwen3"]
    w = _weights("tiny-qwen3", 7)
    base = _runner_prefill_logits(spec, w, IDS)
    seen = []
    real = ops.qk_norm_rope_inplace

    def spy(q, k, pos, cos, sin, qw, kw, eps):
        seen.append((qw, kw, eps))
        assert q.shape[1:] == (8, 16) and k.shape[1:] == (2, 16)
        return real(q, k, pos, cos, sin, torch.ones_like(qw),
                    torch.ones_like(kw), eps)

    monkeypatch.setattr(ops, "qk_norm_rope_inplace", spy)
    moved = _runner_prefill_logits(spec, w, IDS)
    assert len(seen) == spec.n_layers
    for (qw, kw, eps), lw in zip(seen, w.layers):
        assert qw is lw.q_norm and kw is lw.k_norm and eps == spec.rms_eps
    assert (moved - base).abs().max().item() > 1e-3


def test_moe_engine_greedy_deterministic():
    a = _greedy("tiny-qwen3-moe", n=6)
    assert a == _greedy("tiny-qwen3-moe", n=6)


def test_export_supports_qk_norm():
    """The pure-torch export model applies the QK-norm (it must not ignore
    it): its logits equal the runner's."""
    from bee2bee_amd.models.export import ExportableModel

    spec = PRESETS["tiny-qwen3"]
    w = _weights("tiny-qwen3", 7)
    model = ExportableModel(spec, w).eval()
    with torch.no_grad():
        got = model(torch.tensor([IDS]))[0]
    ours = _runner_prefill_logits(spec, w, IDS)
    assert (got - ours).abs().max().item() < 2e-3


def test_legacy_hf_part_chain_applies_qk_norm():
    """The legacy hf_part_* tasks run layer ranges through the same Runner:
    two chained tiny-qwen3 partials equal the full-stack forward."""
    import numpy as np

    from bee2bee_amd.engine.kv import PagedKV
    from bee2bee_amd.engine.runner import Runner
    from bee2bee_amd.legacy.worker import LegacyWorker
    from bee2bee_amd.models.tokenizer import load_tokenizer

    w = LegacyWorker()
    parts = [w.execute_task("hf_part_load", {
        "model_name": "tiny-qwen3", "start": lo, "end": lo + 1, "seed": 5,
    }) for lo in (0, 1)]
    text = "partial forward"
    h0 = w.execute_task("hf_part_forward", {
        "model_id": parts[0]["model_id"], "text": text})["hidden"]
    h1 = w.execute_task("hf_part_forward", {
        "model_id": parts[1]["model_id"], "hidden": h0})["hidden"]

    spec = PRESETS["tiny-qwen3"]
    full = _weights("tiny-qwen3", 5)
    kv = PagedKV(spec, CPU, torch.float32, n_blocks=16)
    runner = Runner(spec, full, kv, CPU, torch.float32)
    tok = load_tokenizer(None, spec.vocab_size, spec.bos_token_id,
                         spec.eos_token_id)
    ids = torch.tensor(tok.encode(text), dtype=torch.int64)
    T = ids.shape[0]
    kv.new_seq(0)
    kv.extend_seq(0, T)
    slots = torch.tensor(kv.slot_mapping(0, range(T)), dtype=torch.int32)
    ref = runner.forward_prefill(
        ids, torch.arange(T, dtype=torch.int32), slots,
        torch.tensor([0, T], dtype=torch.int32), T)
    got = np.array(h1, dtype=np.float32)
    assert np.allclose(got, ref.numpy(), atol=1e-4), \
        np.abs(got - ref.numpy()).max()
