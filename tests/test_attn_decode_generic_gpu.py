"""Decode attention at head sizes other than 64/128: the generic scores
kernel (attn_scores_kernel) followed by attn_pv_kernel, which is what
`path="auto"` launches there.

`max_z=1` is one block per (seq, kv head): FOLD over the three chunks of the
600-key row. `max_z=0` leaves the launcher's rule (Z = C here: partials and
the combine kernel). Inputs come from the fused test's make_case; `out` and
`(m, l)` are checked against ops/reference.py at the tolerances the existing
tests use for the same cache type: assert_close's defaults for bf16,
test_ops_gpu.py::test_fp8_kv_attn_decode's 3e-2 / 3e-2 for fp8, and
assert_ml_close for (m, l).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.ops import reference as R
from tests.test_attn_decode_fused_gpu import (assert_close, assert_ml_close,
                                              make_case)

LENS = [600, 257]
BS = 32


def check(G, hd, max_z, **case_kw):
    q, kc, vc, bt, lens_t, kw = make_case(LENS, G, hd, BS, **case_kw)
    scale = hd ** -0.5
    msg = f"G{G} hd{hd} max_z={max_z} {case_kw}"
    out, ml = ops.attn_decode_select(q, kc, vc, bt, lens_t, scale,
                                     path="auto", max_z=max_z, **kw)
    r_out, r_ml = R.attn_decode_lse(q, kc, vc, bt, lens_t, scale, **kw)
    tol = 3e-2 if case_kw.get("fp8") else 2e-2
    assert_close(out, r_out, atol=tol, rtol=tol, msg=msg)
    assert_ml_close(ml, r_ml, msg=msg)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("max_z", [1, 0])
@pytest.mark.parametrize("G", [1, 4, 16])
@pytest.mark.parametrize("hd", [16, 96])
def test_generic_head_dims(hd, G, max_z, fp8):
    check(G, hd, max_z, fp8=fp8)


@pytest.mark.parametrize("max_z", [1, 0])
@pytest.mark.parametrize("hd", [16, 96])
def test_generic_fp8_scaled(hd, max_z):
    check(4, hd, max_z, fp8=True, scaled=True)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("max_z", [1, 0])
@pytest.mark.parametrize("hd", [16, 96])
def test_generic_window(hd, max_z, fp8):
    check(4, hd, max_z, window=256, fp8=fp8)  # lo = 344 and 1: inside chunks
