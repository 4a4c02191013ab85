"""Per-(layer, kv head) scales for the fp8 KV cache — CPU: the torch
reference ops, the engine's calibration / persistence / checkpoint loading,
and the context-parallel hook. The GPU kernels are checked against these
reference ops in test_kv_scales_gpu.py."""
import json
import multiprocessing as mp
import os
import pickle

import pytest
import torch

from bee2bee_amd.engine.engine import GenerationRequest, InferenceEngine
from bee2bee_amd.engine.sampler import SamplingParams
from bee2bee_amd.ops import reference as R

from tests import kv_scales_common as C

NKV, BS = C.NKV, C.BS


# ------------------------------------------------------------ reference ops


def _empty_cache(nb, hd, dtype=torch.uint8):
    return (torch.zeros(nb, NKV, BS, hd, dtype=dtype),
            torch.zeros(nb, NKV, BS, hd, dtype=dtype))


def _deq(cache):
    return cache.view(torch.float8_e4m3fn).float()


def test_store_clamp():
    """Values beyond 448 * scale saturate to finite +-448 * scale (the
    unscaled reference cast would turn them into NaN)."""
    hd = 16
    scale = torch.tensor([0.5, 0.01, 1.0, 2.0])
    inv = 1.0 / scale
    k = torch.zeros(4, NKV, hd)
    v = torch.zeros(4, NKV, hd)
    lim = 448.0 * scale  # [NKV]
    k[0] = (lim * 3.0).view(NKV, 1)
    k[1] = (-lim * 1.5).view(NKV, 1)
    v[2] = (lim * 1000.0).view(NKV, 1)
    v[3] = (-lim * 1.01).view(NKV, 1)
    kc, vc = _empty_cache(2, hd)
    slots = torch.tensor([3, 40, 17, 5], dtype=torch.int32)
    R.kv_cache_store(k, v, kc, vc, slots, k_inv_scale=inv, v_inv_scale=inv)
    kd = _deq(kc) * scale.view(1, NKV, 1, 1)
    vd = _deq(vc) * scale.view(1, NKV, 1, 1)
    assert torch.isfinite(kd).all() and torch.isfinite(vd).all()
    want = lim.view(NKV, 1).expand(NKV, hd)
    assert torch.equal(kd[0, :, 3], want)
    assert torch.equal(kd[1, :, 8], -want)
    assert torch.equal(vd[0, :, 17], want)
    assert torch.equal(vd[0, :, 5], -want)


def test_unit_scale_identity():
    """inv_scale == 1 on in-range inputs gives the unscaled call's bytes."""
    g = torch.Generator().manual_seed(1)
    hd = 32
    k = torch.randn(40, NKV, hd, generator=g) * 3
    v = torch.randn(40, NKV, hd, generator=g) * 0.02
    slots = torch.randperm(4 * BS, generator=g)[:40].to(torch.int32)
    ones = torch.ones(NKV)
    kc, vc = _empty_cache(4, hd)
    kc1, vc1 = _empty_cache(4, hd)
    R.kv_cache_store(k, v, kc, vc, slots)
    R.kv_cache_store(k, v, kc1, vc1, slots, k_inv_scale=ones,
                     v_inv_scale=ones)
    assert torch.equal(kc, kc1) and torch.equal(vc, vc1)
    # and reading with unit scales is reading without
    q = torch.randn(1, NKV * 2, hd, generator=g)
    bt = torch.arange(4, dtype=torch.int32).view(1, 4)
    lens = torch.tensor([100], dtype=torch.int32)
    a = R.attn_decode(q, kc, vc, bt, lens, hd**-0.5)
    b = R.attn_decode(q, kc, vc, bt, lens, hd**-0.5, k_scale=ones,
                      v_scale=ones)
    assert torch.equal(a, b)


def test_scales_need_fp8_cache():
    hd = 16
    k = torch.zeros(1, NKV, hd)
    kc, vc = _empty_cache(1, hd, dtype=torch.float32)
    ones = torch.ones(NKV)
    slots = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        R.kv_cache_store(k, k, kc, vc, slots, k_inv_scale=ones,
                         v_inv_scale=ones)
    q = torch.zeros(1, NKV, hd)
    bt = torch.zeros(1, 1, dtype=torch.int32)
    lens = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        R.attn_decode(q, kc, vc, bt, lens, 1.0, k_scale=ones, v_scale=ones)


@pytest.fixture(scope="module")
def outlier():
    """The shared outlier input as three caches of the same K/V: fp32
    (truth), scaled fp8 (scale = per-head amax / 448) and today's unscaled
    fp8. Two sequences (300 / 77 tokens), permuted block table, block 0
    unused."""
    g = torch.Generator().manual_seed(21)
    B, G, hd = 2, 4, 128
    lens = torch.tensor([300, 77], dtype=torch.int32)
    W = -(-300 // BS)
    bt, nb = C.permuted_block_table(B, W, g)
    k, v = C.outlier_kv(nb * BS, hd, g)
    ks, vs, kis, vis = C.amax_scales(k, v)
    slots = torch.arange(nb * BS, dtype=torch.int32)
    kc32, vc32 = _empty_cache(nb, hd, dtype=torch.float32)
    R.kv_cache_store(k, v, kc32, vc32, slots)
    kcs, vcs = _empty_cache(nb, hd)
    R.kv_cache_store(k, v, kcs, vcs, slots, k_inv_scale=kis, v_inv_scale=vis)
    kcu, vcu = _empty_cache(nb, hd)
    R.kv_cache_store(k, v, kcu, vcu, slots)  # head 0 overflows to NaN
    return dict(B=B, G=G, hd=hd, lens=lens, bt=bt, ks=ks, vs=vs,
                truth=(kc32, vc32), scaled=(kcs, vcs), unit=(kcu, vcu),
                scale=hd**-0.5)


def _qgen():
    return torch.Generator().manual_seed(22)


def _check_bound(err_scaled, err_unit, what):
    """Every kv head under scaled fp8 within 2x of head 2 (unit magnitude)
    under today's unscaled fp8. 2x covers amax landing anywhere in a
    binade."""
    base = float(err_unit[2])
    print(f"{what}: scaled rel-L2 per head {err_scaled.tolist()}, "
          f"unscaled {err_unit.tolist()}, baseline (head 2) {base}")
    assert base > 0 and base == base
    for h in range(NKV):
        assert float(err_scaled[h]) <= 2.0 * base, (what, h, err_scaled, base)


def test_accuracy_decode_vs_truth(outlier):
    o = outlier
    q = C.outlier_q(o["B"], o["G"], o["hd"], _qgen())
    args = (o["bt"], o["lens"], o["scale"])
    truth = R.attn_decode(q, *o["truth"], *args)
    got = R.attn_decode(q, *o["scaled"], *args, k_scale=o["ks"],
                        v_scale=o["vs"])
    unit = R.attn_decode(q, *o["unit"], *args)
    assert torch.isfinite(got).all()
    _check_bound(C.rel_l2_per_head(got, truth, o["G"]),
                 C.rel_l2_per_head(unit, truth, o["G"]), "decode")
    # what the scales buy: unscaled, the large head is garbage and the
    # small head visibly worse than the unit-magnitude ones
    e_unit = C.rel_l2_per_head(unit, truth, o["G"])
    assert not float(e_unit[0]) <= 2.0 * float(e_unit[2])
    assert float(e_unit[1]) > 2.0 * float(e_unit[2])


def test_accuracy_lse_vs_truth(outlier):
    o = outlier
    q = C.outlier_q(o["B"], o["G"], o["hd"], _qgen())
    args = (o["bt"], o["lens"], o["scale"])

    def lse(ml):  # [B, nq, 2] -> [B, nq, 1]: log of the softmax denominator
        return (ml[..., 0] + torch.log(ml[..., 1])).unsqueeze(-1)

    _o, ml_t = R.attn_decode_lse(q, *o["truth"], *args)
    _o, ml_s = R.attn_decode_lse(q, *o["scaled"], *args, k_scale=o["ks"],
                                 v_scale=o["vs"])
    _o, ml_u = R.attn_decode_lse(q, *o["unit"], *args)
    _check_bound(C.rel_l2_per_head(lse(ml_s), lse(ml_t), o["G"]),
                 C.rel_l2_per_head(lse(ml_u), lse(ml_t), o["G"]), "lse")


def test_accuracy_chunked_prefill_vs_truth(outlier):
    o = outlier
    qlens = torch.tensor([70, 64], dtype=torch.int32)  # chunks ending at L
    q = C.outlier_q(int(qlens.sum()), o["G"], o["hd"], _qgen())
    args = (o["bt"], o["lens"], qlens, o["scale"])
    truth = R.attn_decode_with_history(q, *o["truth"], *args)
    got = R.attn_decode_with_history(q, *o["scaled"], *args,
                                     k_scale=o["ks"], v_scale=o["vs"])
    unit = R.attn_decode_with_history(q, *o["unit"], *args)
    _check_bound(C.rel_l2_per_head(got, truth, o["G"]),
                 C.rel_l2_per_head(unit, truth, o["G"]), "chunked prefill")


# ------------------------------------------------------------------ engine


def _tiny(**kw):
    kw.setdefault("max_batch", 2)
    kw.setdefault("max_seq_len", 128)
    kw.setdefault("seed", 7)
    return InferenceEngine("tiny", device="cpu", **kw)


def _rewrite_v_outlier(eng, factor=2000.0):
    """Function-preserving rewrite: scale kv head 0's V projection rows up
    and the wo input columns of its q heads down by the same factor."""
    s = eng.spec
    G = s.n_heads // s.n_kv_heads
    v0 = s.q_size + s.kv_size  # first V row of kv head 0 in wqkv
    for lw in eng.weights.layers:
        lw.wqkv[v0: v0 + s.head_dim] *= factor
        if lw.wqkv_bias is not None:
            lw.wqkv_bias[v0: v0 + s.head_dim] *= factor
        lw.wo[:, : G * s.head_dim] /= factor


def _chunked_hidden(eng, ids, chunk=16):
    """Runner.forward_prefill in chunks against the paged history, so every
    chunk after the first reads the cache. Returns all final-hidden rows."""
    kv, seq = eng.kv, 1000
    kv.new_seq(seq)
    rows = []
    try:
        for start in range(0, len(ids), chunk):
            take = min(chunk, len(ids) - start)
            kv.extend_seq(seq, start + take)
            pos = range(start, start + take)
            with torch.no_grad():
                h = eng.runner.forward_prefill(
                    torch.tensor(ids[start: start + take], dtype=torch.int64),
                    torch.tensor(list(pos), dtype=torch.int32),
                    torch.tensor(kv.slot_mapping(seq, pos), dtype=torch.int32),
                    torch.tensor([0, take], dtype=torch.int32), take,
                    block_table=kv.block_table([seq]),
                    seq_lens=torch.tensor([start + take], dtype=torch.int32),
                    query_lens=torch.tensor([take], dtype=torch.int32),
                )
            rows.append(h.float())
    finally:
        kv.free_seq(seq)
    return torch.cat(rows)


def test_outlier_rewrite_calibrated_matches_unit_on_plain_model():
    ids = [(i * 37 + 11) % 500 + 4 for i in range(80)]
    calib = [ids, [(i * 13 + 5) % 500 + 4 for i in range(60)]]

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    engs = []
    try:
        # today's unit-scale fp8 on the unrewritten model
        native, unit8 = _tiny(), _tiny(kv_dtype="fp8")
        engs += [native, unit8]
        err_unit = rel(_chunked_hidden(unit8, ids),
                       _chunked_hidden(native, ids))
        # calibrated fp8 on the rewritten model (V of kv head 0 x2000)
        native_rw, cal8 = _tiny(), _tiny(kv_dtype="fp8")
        engs += [native_rw, cal8]
        _rewrite_v_outlier(native_rw)
        _rewrite_v_outlier(cal8)
        cal8.calibrate_kv_scales(calib)
        assert cal8.stats()["kv_scales"] == "calibrated"
        err_cal = rel(_chunked_hidden(cal8, ids),
                      _chunked_hidden(native_rw, ids))
        print(f"final-hidden rel-L2: unit/plain {err_unit}, "
              f"calibrated/rewritten {err_cal}")
        assert err_unit > 0
        assert err_cal <= 2.0 * err_unit, (err_cal, err_unit)
        ratio = cal8.kv.v_scale[:, 0] / cal8.kv.v_scale[:, 1]
        assert bool((ratio > 100).all()), ratio
        # reciprocals are kept in step
        assert torch.equal(cal8.kv.v_inv_scale, 1.0 / cal8.kv.v_scale)
        assert torch.equal(cal8.kv.k_inv_scale, 1.0 / cal8.kv.k_scale)
    finally:
        for e in engs:
            e.shutdown()


def test_scale_file_roundtrip_and_mismatch(tmp_path):
    eng = _tiny(kv_dtype="fp8")
    path = str(tmp_path / "scales.json")
    try:
        eng.calibrate_kv_scales([[5, 6, 7, 8, 9, 10, 11, 12]], margin=1.7)
        eng.save_kv_scales(path)
        eng2 = _tiny(kv_dtype="fp8", kv_scales=path)
        try:
            assert eng2.stats()["kv_scales"] == "file"
            for name in ("k_scale", "v_scale", "k_inv_scale", "v_inv_scale"):
                assert torch.equal(getattr(eng2.kv, name),
                                   getattr(eng.kv, name)), name
        finally:
            eng2.shutdown()
    finally:
        eng.shutdown()
    with open(path) as f:
        doc = json.load(f)
    assert doc["model"] == "tiny" and doc["n_kv_heads"] == eng.spec.n_kv_heads
    # a file for another head count fails loudly
    doc["n_kv_heads"] += 1
    doc["k_scale"] = [row + [1.0] for row in doc["k_scale"]]
    doc["v_scale"] = [row + [1.0] for row in doc["v_scale"]]
    bad = str(tmp_path / "bad.json")
    with open(bad, "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match="n_kv_heads"):
        _tiny(kv_dtype="fp8", kv_scales=bad)
    # scales without an fp8 cache: a clear error, not silently ignored
    with pytest.raises(ValueError, match="fp8"):
        _tiny(kv_scales=path)


def test_scales_frozen_while_sequences_live():
    eng = _tiny(kv_dtype="fp8")
    try:
        ones = torch.ones_like(eng.kv.k_scale)
        eng.kv.set_scales(ones * 2, ones * 3)  # only the scratch seq: fine
        eng.kv.new_seq(5)
        eng.kv.extend_seq(5, 3)
        with pytest.raises(RuntimeError):
            eng.kv.set_scales(ones, ones)
        with pytest.raises(RuntimeError):
            eng.calibrate_kv_scales([[1, 2, 3]])
        assert torch.equal(eng.kv.k_scale, ones * 2)  # untouched
        eng.kv.free_seq(5)
        # a queued request blocks calibration too
        eng._pending.put(GenerationRequest(prompt_ids=[1, 2]))
        with pytest.raises(RuntimeError):
            eng.calibrate_kv_scales([[1, 2, 3]])
        eng._pending.get_nowait()
        eng.calibrate_kv_scales([[1, 2, 3]])
    finally:
        eng.shutdown()


def test_checkpoint_scales(tmp_path):
    from safetensors.torch import save_file

    from bee2bee_amd.models.weights import save_hf

    src = _tiny()
    ckpt = str(tmp_path / "ckpt")
    try:
        save_hf(src.weights, ckpt)
        spec = src.spec
    finally:
        src.shutdown()

    # the same checkpoint without scales loads as before
    plain = _tiny(model_path=ckpt, kv_dtype="fp8")
    try:
        assert plain.weights.kv_scales is None
        assert plain.stats()["kv_scales"] == "unit"
    finally:
        plain.shutdown()
    with pytest.raises(ValueError, match="checkpoint"):
        _tiny(model_path=ckpt, kv_dtype="fp8", kv_scales="checkpoint")

    extra = {}
    for i in range(spec.n_layers):
        pfx = f"model.layers.{i}.self_attn"
        extra[f"{pfx}.k_scale"] = torch.tensor(0.25 + i)  # scalar
        extra[f"{pfx}.v_scale"] = (
            torch.arange(1, spec.n_kv_heads + 1, dtype=torch.float32)
            * 0.5 + i)  # per kv head
    save_file(extra, os.path.join(ckpt, "model-kv-scales.safetensors"))
    eng = _tiny(model_path=ckpt, kv_dtype="fp8", kv_scales="checkpoint")
    try:
        assert eng.stats()["kv_scales"] == "checkpoint"
        for i in range(spec.n_layers):
            assert torch.equal(eng.kv.k_scale[i],
                               torch.full((spec.n_kv_heads,), 0.25 + i))
            assert torch.equal(eng.kv.v_scale[i],
                               extra[f"model.layers.{i}.self_attn.v_scale"])
        assert torch.equal(eng.kv.k_inv_scale, 1.0 / eng.kv.k_scale)
        r = eng.generate([5, 6, 7, 8], max_new_tokens=3, temperature=0.0,
                         repetition_penalty=1.0)
        assert len(r.output_ids) == 3
    finally:
        eng.shutdown()


def test_uncalibrated_fp8_engine_has_unit_scales():
    eng = _tiny(kv_dtype="fp8")
    try:
        s = eng.spec
        for name in ("k_scale", "v_scale", "k_inv_scale", "v_inv_scale"):
            t = getattr(eng.kv, name)
            assert t.dtype == torch.float32
            assert tuple(t.shape) == (s.n_layers, s.n_kv_heads)
            assert bool((t == 1.0).all())
        assert eng.stats()["kv_scales"] == "unit"
        assert eng.stats()["kv_dtype"] == "fp8"
    finally:
        eng.shutdown()
    native = _tiny()
    try:
        assert native.kv.k_scale is None
        assert native.kv.layer_scales(0) is None
    finally:
        native.shutdown()


def test_calibration_reaches_decode_and_chunked_prefill():
    """After calibration the engine serves end to end (chunked prefill +
    decode read the scaled cache) and stays finite."""
    eng = _tiny(kv_dtype="fp8", max_prefill_tokens=16)
    try:
        prompt = [(i * 7 + 3) % 500 for i in range(40)]
        eng.calibrate_kv_scales([prompt])
        r = GenerationRequest(prompt_ids=list(prompt), max_new_tokens=6,
                              sampling=SamplingParams(greedy=True))
        eng.submit(r)
        while True:
            x = r.out_queue.get(timeout=60)
            if not isinstance(x, int):
                break
        assert r.error is None, r.error
        assert len(r.output_ids) == 6
    finally:
        eng.shutdown()


def test_cli_rejects_scales_without_fp8(monkeypatch):
    from click.testing import CliRunner

    from bee2bee_amd.__main__ import cli

    monkeypatch.delenv("BEE2BEE_KV_FP8", raising=False)
    res = CliRunner().invoke(cli, ["serve-native", "--kv-scales", "calibrate"])
    assert res.exit_code != 0
    assert "--kv-fp8" in res.output


# ------------------------------------------------------ context parallelism

CP_B, CP_NKV, CP_G, CP_HD, CP_PAGE = 3, 2, 2, 64, 16
CP_SCALE = CP_HD ** -0.5


def _cp_ctx(seed=7, n_pages_total=64):
    """test_cp_cpu.py's context, with per-head K/V magnitudes 4 / 0.05 and a
    scaled fp8 cache (scale = per-head amax / 448)."""
    g = torch.Generator().manual_seed(seed)
    std = torch.tensor([4.0, 0.05]).view(1, CP_NKV, 1)
    q = torch.randn(CP_B, CP_NKV * CP_G, CP_HD, generator=g)
    k = torch.randn(n_pages_total * CP_PAGE, CP_NKV, CP_HD, generator=g) * std
    v = torch.randn(n_pages_total * CP_PAGE, CP_NKV, CP_HD, generator=g) * std
    ks = k.abs().amax(dim=(0, 2)) / 448.0
    vs = v.abs().amax(dim=(0, 2)) / 448.0
    kc = torch.zeros(n_pages_total, CP_NKV, CP_PAGE, CP_HD, dtype=torch.uint8)
    vc = torch.zeros_like(kc)
    R.kv_cache_store(k, v, kc, vc,
                     torch.arange(n_pages_total * CP_PAGE, dtype=torch.int32),
                     k_inv_scale=1.0 / ks, v_inv_scale=1.0 / vs)
    seq_lens = torch.tensor([250, 37, 129], dtype=torch.int32)
    W = -(-int(seq_lens.max()) // CP_PAGE)
    bt = torch.arange(CP_B * W, dtype=torch.int32).reshape(CP_B, W)
    return q, kc, vc, bt, seq_lens, ks, vs


def _cp_scaled_worker(rank, world, port, out_path):
    import torch.distributed as dist

    from bee2bee_amd.parallel.cp import (cp_attn_decode, local_lens,
                                         shard_pages)

    dist.init_process_group(
        backend="gloo", init_method=f"tcp://127.0.0.1:{port}",
        rank=rank, world_size=world,
    )
    try:
        q, kc, vc, bt, seq_lens, ks, vs = _cp_ctx()
        lls = local_lens(seq_lens, CP_PAGE, world, rank)
        lbt = torch.zeros_like(bt)
        for i, L in enumerate(seq_lens.tolist()):
            n_pages = -(-L // CP_PAGE)
            lo, hi = shard_pages(n_pages, world, rank)
            lbt[i, : hi - lo] = bt[i, lo:hi]
        out = cp_attn_decode(q, kc, vc, lbt, lls, CP_SCALE, k_scale=ks,
                             v_scale=vs)
        if rank == 0:
            with open(out_path, "wb") as f:
                pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_cp2_gloo_scaled_fp8_matches_single(tmp_path):
    q, kc, vc, bt, seq_lens, ks, vs = _cp_ctx()
    full = R.attn_decode(q, kc, vc, bt, seq_lens, CP_SCALE, k_scale=ks,
                         v_scale=vs)
    # the scales matter here: without them the result is a different one
    assert not torch.allclose(
        full, R.attn_decode(q, kc, vc, bt, seq_lens, CP_SCALE), atol=1e-2)
    out_path = str(tmp_path / "cp.pkl")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_cp_scaled_worker,
                         args=(r, 2, 29883, out_path)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=200)
        assert p.exitcode == 0
    with open(out_path, "rb") as f:
        got = pickle.load(f)
    assert torch.allclose(got.float(), full.float(), atol=1e-5)
