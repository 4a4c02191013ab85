"""Tensor parallelism for the Qwen3 family on CPU (gloo, world 2): the
per-head_dim q_norm / k_norm weights are replicated on every rank, and TP2
greedy decode matches the single-process engine. tiny-qwen3 has q_size 128
over hidden 64, so a shard that sliced by hidden_size would break here."""
import multiprocessing as mp
import pickle

import pytest
import torch

from bee2bee_amd.models.spec import PRESETS

PROMPTS = [[5, 6, 7, 8, 9], [100, 101]]
N_NEW = 6
SEED = 31
MODEL = "tiny-qwen3"


def test_shard_weights_replicates_qk_norm():
    from bee2bee_amd.models.weights import ModelWeights
    from bee2bee_amd.parallel.tp import shard_spec, shard_weights

    spec = PRESETS[MODEL]  # 8 q heads, 2 kv heads, hd 16, hidden 64
    full = ModelWeights(spec, torch.device("cpu"), torch.float32).random_init(SEED)
    lspec = shard_spec(spec, 2)
    assert lspec.qk_norm and lspec.q_size == 64 and lspec.kv_size == 16
    for rank in range(2):
        sh = shard_weights(full, spec, rank, 2)
        for li in range(spec.n_layers):
            assert torch.equal(sh.layers[li].q_norm, full.layers[li].q_norm)
            assert torch.equal(sh.layers[li].k_norm, full.layers[li].k_norm)
            assert sh.layers[li].q_norm.shape == (spec.head_dim,)
        assert sh.layers[0].wqkv.shape == (lspec.q_size + 2 * lspec.kv_size,
                                           spec.hidden_size)
        assert sh.layers[0].wo.shape == (spec.hidden_size, lspec.q_size)
    s1 = shard_weights(full, spec, 1, 2)
    assert torch.equal(s1.layers[0].wqkv[0],
                       full.layers[0].wqkv[spec.q_size // 2])


def _tp_worker(rank: int, world: int, port: int, out_path: str) -> None:
    import torch.distributed as dist

    from bee2bee_amd.parallel.tp import TPEngine

    dist.init_process_group(
        backend="gloo",
        init_method=f"tcp://127.0.0.1:{port}",
        rank=rank,
        world_size=world,
    )
    try:
        eng = TPEngine(MODEL, device="cpu", max_batch=4, max_seq_len=64,
                       seed=SEED)
        outs = eng.generate(PROMPTS, N_NEW)
        if rank == 0:
            with open(out_path, "wb") as f:
                pickle.dump(outs, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_tp2_matches_single_process(tmp_path):
    out_path = str(tmp_path / "tp_out.pkl")
    ctx = mp.get_context("spawn")
    procs = [
        ctx.Process(target=_tp_worker, args=(r, 2, 29733, out_path))
        for r in range(2)
    ]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0, f"tp worker failed (exit {p.exitcode})"
    with open(out_path, "rb") as f:
        tp_outs = pickle.load(f)

    from bee2bee_amd.engine.engine import GenerationRequest, InferenceEngine
    from bee2bee_amd.engine.sampler import SamplingParams

    eng = InferenceEngine(MODEL, device="cpu", max_batch=4, max_seq_len=64,
                          seed=SEED)
    try:
        ref = []
        for prompt in PROMPTS:
            req = GenerationRequest(
                prompt_ids=list(prompt), max_new_tokens=N_NEW,
                sampling=SamplingParams(greedy=True),
            )
            eng.submit(req)
            while True:
                item = req.out_queue.get(timeout=60)
                if not isinstance(item, int):
                    break
            ref.append(req.output_ids)
    finally:
        eng.shutdown()
    assert tp_outs == ref
