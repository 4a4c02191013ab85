"""Seeded per-request sampling on the CPU engine (`tiny`, fp32 reference
ops): a seeded request's tokens are a function of the request alone, and
`seed` travels every interface down to the sampling parameters."""
import json

import pytest
from fastapi.testclient import TestClient

from bee2bee_amd import ops
from bee2bee_amd.engine.engine import GenerationRequest, InferenceEngine
from bee2bee_amd.engine.sampler import SamplingParams, sanitize_seed
from bee2bee_amd.mesh import wire

PROMPT = [3 + (7 * i) % 200 for i in range(20)]
KEY = {"X-API-KEY": "secret-key"}


def _engine(**kw):
    kw.setdefault("max_batch", 8)
    return InferenceEngine("tiny", device="cpu", max_seq_len=128, seed=7,
                           **kw)


def _req(prompt, n=32, **knobs):
    knobs.setdefault("temperature", 0.8)
    return GenerationRequest(
        prompt_ids=list(prompt), max_new_tokens=n,
        sampling=SamplingParams.from_request(
            knobs.pop("temperature"), knobs.pop("top_p", None),
            knobs.pop("top_k", None), knobs.pop("repetition_penalty", None),
            knobs.pop("seed", None)))


def _drain(req):
    while isinstance(req.out_queue.get(timeout=120), int):
        pass
    assert req.error is None, req.error
    return list(req.output_ids)


# seven neighbours with other parameters; some seeded, some greedy
_OTHERS = [
    dict(temperature=0.0, repetition_penalty=1.0),
    dict(temperature=1.2, top_k=8, seed=5),
    dict(temperature=0.7, top_p=0.5, repetition_penalty=1.3),
    dict(temperature=1.0, top_k=200, seed=99, repetition_penalty=1.0),
    dict(temperature=0.0),
    dict(temperature=0.9, top_k=0, seed=3),
    dict(temperature=0.6, top_k=3),
]


def _among_others(eng, place, **target):
    """Submit the target at position `place` among the seven others."""
    reqs = []
    for i, knobs in enumerate(_OTHERS):
        if i == place:
            reqs.append(eng.submit(_req(PROMPT, **target)))
        reqs.append(eng.submit(_req([11 + i, 5, 9 + 2 * i] * (1 + i % 3),
                                    n=8 + 5 * i, **knobs)))
    outs = [_drain(r) for r in reqs]
    return outs[place]


@pytest.fixture(scope="module")
def solo():
    eng = _engine()
    try:
        yield _drain(eng.submit(_req(PROMPT, seed=1234)))
    finally:
        eng.shutdown()


def test_seeded_request_is_batch_invariant(solo):
    assert len(solo) == 32
    eng = _engine()
    try:
        # the same engine again: nothing carries over between requests
        assert _drain(eng.submit(_req(PROMPT, seed=1234))) == solo
        assert _among_others(eng, 3, seed=1234) == solo
        assert _among_others(eng, 0, seed=1234) == solo
    finally:
        eng.shutdown()


def test_seeded_request_survives_chunked_prefill(solo):
    eng = _engine(max_prefill_tokens=8)   # the 20-token prompt takes 3 steps
    try:
        assert _drain(eng.submit(_req(PROMPT, seed=1234))) == solo
        assert _among_others(eng, 5, seed=1234) == solo
    finally:
        eng.shutdown()


def test_seeds_differ_and_wrap(solo):
    eng = _engine()
    try:
        assert _drain(eng.submit(_req(PROMPT, seed=1235))) != solo
        # seeds are taken mod 2^64
        assert _drain(eng.submit(_req(PROMPT, seed=1234 + 2 ** 64))) == solo
        hi = _drain(eng.submit(_req(PROMPT, seed=2 ** 63 + 1234)))
        assert hi != solo and len(hi) == 32
    finally:
        eng.shutdown()


def test_seeded_top_k_outside_the_kernel_range_is_served_with_1024():
    eng = _engine()
    try:
        a = _drain(eng.submit(_req(PROMPT, seed=8, top_k=0)))
        b = _drain(eng.submit(_req(PROMPT, seed=8, top_k=1024)))
        c = _drain(eng.submit(_req(PROMPT, seed=8, top_k=5000)))
        assert a == b == c
    finally:
        eng.shutdown()


def test_fused_sampler_rows_equal_their_solo_runs():
    """fused_sampler on: eligible unseeded requests draw a seed at submit
    from the engine seed, so the same submissions give the same tokens;
    seeded ones equal their solo runs in any mix."""
    def mix(eng):
        reqs = [eng.submit(_req([9 + i, 4, 6] * 2, n=12, **knobs))
                for i, knobs in enumerate(_OTHERS)]
        return [_drain(r) for r in reqs]

    e1, e2 = _engine(fused_sampler=True), _engine(fused_sampler=True)
    try:
        assert e1.fused_sampler and mix(e1) == mix(e2)
        seeded = [i for i, k in enumerate(_OTHERS) if "seed" in k]
        out = mix(e1)
        for i in seeded:
            alone = _drain(e2.submit(_req([9 + i, 4, 6] * 2, n=12,
                                          **_OTHERS[i])))
            assert alone == out[i]
    finally:
        e1.shutdown()
        e2.shutdown()


def test_default_path_never_calls_sample_rows(monkeypatch):
    """Option off, no seed: the grouped torch path, as before."""
    def boom(*a, **k):
        raise AssertionError("ops.sample_rows called on the default path")

    monkeypatch.setattr(ops, "sample_rows", boom)
    monkeypatch.delenv("BEE2BEE_FUSED_SAMPLER", raising=False)
    eng = _engine()
    try:
        assert not eng.fused_sampler
        reqs = [eng.submit(_req([5, 6, 7], n=6, **{
            k: v for k, v in knobs.items() if k != "seed"}))
            for knobs in _OTHERS]
        assert all(len(_drain(r)) == 6 for r in reqs)
        # and a seed does reach it: one call per token
        calls = []
        real = ops.reference.sample_rows

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)

        monkeypatch.setattr(ops, "sample_rows", counting)
        assert len(_drain(eng.submit(_req([5, 6, 7], n=3, seed=1)))) == 3
        assert len(calls) == 3
    finally:
        eng.shutdown()


def test_env_switches_the_fused_sampler_on(monkeypatch):
    monkeypatch.setenv("BEE2BEE_FUSED_SAMPLER", "1")
    eng = _engine(max_batch=2)
    try:
        assert eng.fused_sampler
    finally:
        eng.shutdown()


# ------------------------------------------------------------- interfaces

def test_hostile_seeds_sanitise_to_none():
    for bad in ("abc", "12", float("nan"), float("inf"), -float("inf"), 1.5,
                True, False, [1], {"a": 1}, None, b"7"):
        assert sanitize_seed(bad) is None, bad
        assert SamplingParams.from_request(0.7, seed=bad).seed is None
    assert sanitize_seed(0) == 0
    assert sanitize_seed(7.0) == 7
    assert sanitize_seed(-1) == 2 ** 64 - 1
    assert sanitize_seed(2 ** 64 + 3) == 3
    assert sanitize_seed(10 ** 40) == 10 ** 40 % 2 ** 64
    sp = SamplingParams.from_request(0.7, 0.9, 40, 1.1, 42)
    assert (sp.seed, sp.top_k, sp.top_p) == (42, 40, 0.9)
    assert SamplingParams.from_request(0.7).seed is None


def test_seed_rides_the_wire_frame():
    frame = wire.gen_request("r1", "p", "m", sampling={"seed": 77,
                                                       "top_k": 40})
    assert frame["seed"] == 77
    params = wire.request_params(json.loads(json.dumps(frame)))
    assert params["seed"] == 77 and params["top_k"] == 40
    # an absent key means unseeded; old peers never see the key
    frame2 = wire.gen_request("r2", "p", "m", sampling={"seed": None})
    assert "seed" not in frame2
    assert "seed" not in wire.request_params(frame2)
    assert "seed" not in wire.gen_request("r3", "p", "m")
    assert "seed" in wire.SAMPLING_KEYS


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setenv("BEE2BEE_API_KEY", "secret-key")
    monkeypatch.setenv("BEE2BEE_DISABLE_NAT", "1")
    monkeypatch.setenv("BEE2BEE_PORT", "0")
    monkeypatch.setenv("BEE2BEE_HOST", "127.0.0.1")
    monkeypatch.delenv("BEE2BEE_BOOTSTRAP", raising=False)
    from bee2bee_amd.gateway import api as gateway_api

    gateway_api.node = None
    with TestClient(gateway_api.app) as c:
        yield c
    gateway_api.node = None


def _capture_service():
    from bee2bee_amd.gateway import api as gateway_api
    from tests.test_mesh import EchoService

    class Capture(EchoService):
        def execute(self, params):
            self.last_params = params
            return super().execute(params)

        def execute_stream(self, params):
            self.last_params = params
            return super().execute_stream(params)

    svc = Capture(model="cap-model")
    gateway_api.node.local_services[svc.name] = svc
    return svc


@pytest.mark.parametrize("route,body", [
    ("/generate", {"prompt": "hi"}),
    ("/chat", {"prompt": "hi"}),
    ("/v1/completions", {"prompt": "hi"}),
    ("/v1/chat/completions",
     {"messages": [{"role": "user", "content": "hi"}]}),
])
def test_seed_reaches_the_service_from_every_route(client, route, body):
    svc = _capture_service()
    body = dict(body, model="cap-model")
    r = client.post(route, headers=KEY, json=dict(body, seed=4242))
    assert r.status_code == 200, r.text
    assert svc.last_params["seed"] == 4242
    # absent stays absent (or None): the request is unseeded
    r = client.post(route, headers=KEY, json=body)
    assert r.status_code == 200
    assert svc.last_params.get("seed") is None
    # a hostile value is not a client error; the service sanitises it
    r = client.post(route, headers=KEY, json=dict(body, seed="zzz"))
    assert r.status_code == 200


def test_seed_reaches_the_service_from_the_streaming_routes(client):
    svc = _capture_service()
    for route, body in (
            ("/v1/completions", {"prompt": "hi"}),
            ("/v1/chat/completions",
             {"messages": [{"role": "user", "content": "hi"}]})):
        svc.last_params = None
        with client.stream("POST", route, headers=KEY, json=dict(
                body, model="cap-model", seed=9, stream=True)) as r:
            assert r.status_code == 200
            list(r.iter_lines())
        assert svc.last_params["seed"] == 9


def test_native_service_takes_the_seed():
    from bee2bee_amd.services.native import NativeEngineService

    svc = NativeEngineService("tiny", device="cpu", max_batch=2,
                              max_seq_len=128)
    svc.load_sync()
    try:
        _, _, _, extra = svc._check({"prompt": "x", "seed": 2 ** 64 + 5})
        assert extra["seed"] == 5
        _, _, _, extra = svc._check({"prompt": "x", "seed": "nope"})
        assert "seed" not in extra
        p = {"prompt": "hello there", "max_new_tokens": 12,
             "temperature": 0.9, "seed": 31}
        a, b = svc.execute(p), svc.execute(p)
        assert a["text"] == b["text"] and a["tokens"] == b["tokens"]
        streamed = "".join(
            json.loads(line).get("text", "")
            for line in svc.execute_stream(p))
        assert streamed == a["text"]
    finally:
        svc.engine.shutdown()
