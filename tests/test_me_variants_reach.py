"""The parameter variants of tests/test_gpu_me.py::test_me_frame_param_variants reach the rules they are there for: on the oracle
alone, a variant's outputs differ from the outputs of the same clip and parameter set with the variant's override undone.  (A
variant that changes nothing would pass the GPU comparison whatever the kernel did with its parameters.)"""
import numpy as np
import pytest

import me_cases


def oracle_outputs(orc, v, _cache={}, **kw):
    prm = me_cases.variant_params(v, **kw)
    key = (v.clip, repr(v.refs), bytes(prm))
    if key not in _cache:
        pyrs, w, h = me_cases.variant_clip(orc, v)
        cur, l0, l1 = v.refs
        _cache[key] = me_cases.run_cpu(orc.orc_me_frame_range, prm, pyrs, cur, l0, l1, w, h)
    return _cache[key]


def differing(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


@pytest.mark.parametrize("v", [v for v in me_cases.PARAM_VARIANTS if v.over], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.over.items()))
def test_variant_changes_the_oracle_output(orc, v):
    assert differing(oracle_outputs(orc, v), oracle_outputs(orc, v, undo=True)), v
    if v.over.get("enable_me_sr_adjustment") == 2:  # the rules of the value 2, not those the value 1 shares with it
        assert differing(oracle_outputs(orc, v), oracle_outputs(orc, v, enable_me_sr_adjustment=1)), v
