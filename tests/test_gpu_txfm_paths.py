"""GPU parity of the fused transform kernel (csrc/txfm_block.hpp behind svt_hip_txfm_quant_batch) and of
svt_hip_quantize_batch on every path the data can choose, bit-exact against the oracle pipeline orc_fwd_txfm2d ->
orc_handle_transform64 -> tx_cases.orc_quant -> orc_inv_txfm2d_add, orc_full_distortion32 and orc_satd.

The kernel picks its quantiser per wavefront from the data (quant_small<true>, quant_small<false> or the general quant_one)
and its coefficient stores from the alignment of the output.  tx_cases.path_cases lays the blocks out in runs of one
wavefront each with a known composition; tx_cases.path_census states which path each wave takes, and the census is asserted
here and, without a GPU, in test_txfm_path_census.py.  Sizes with a 64-point side hold one block per wave, so no wave of
theirs can mix the two quantiser families: that class is empty there by construction.  A 4x4 block of 10-bit samples cannot
produce a coefficient above 32767 (the largest is 32 * 1023), so the blocks meant to leave int16 are 12-bit where 10 bits do
not get there.  Two kinds of block are aimed at single lines of the kernel: 'edge' blocks keep every coefficient within int16
but |DC| + round beyond it, inside a short-form wave, so the saturation of QUANT_B / QUANT_FP there decides the result; 'over'
blocks carry a DC between 32768 and 65535 and the largest quant the tables take, for which the 32-bit products of the short
form would overflow, so the 32767 bound of the path choice decides it."""
import ctypes as C

import numpy as np
import pytest

import tx_cases as T
from arena import GUARD, check_containment
from svtav1_hip import abi, device
from tx_cases import V

pytestmark = pytest.mark.gpu
_RUNS = {}


def run_fused(hip, w, h, batch, distortion=False):
    """-> (arena after svt_hip_txfm_quant_batch, results (n, 16) bytes, svt_hip_txfm_distortion_batch's output or None)"""
    arena, darr = batch["arena"], batch["descs"]
    n_tb = len(darr)
    darena = device.DeviceBuffer(hip, arena.nbytes + 256)
    darena.upload(arena)
    ddesc = device.DeviceBuffer(hip, C.sizeof(darr))
    ddesc.upload(np.frombuffer(darr, dtype=np.uint8))
    dres = device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_tb)
    dres.fill(GUARD)
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    device.check(hip, hip.svt_hip_txfm_quant_batch(V(darena.ptr), V(ddesc.ptr), V(dres.ptr), C.c_uint32(n_tb), C.c_uint32(w),
                                                   C.c_uint32(h), None), "svt_hip_txfm_quant_batch")
    out = darena.download(np.uint8, (arena.nbytes,))
    res_raw = dres.download(np.uint8, (n_tb, abi.TXFM_RESULT_BYTES))
    dist = None
    if distortion:
        ddist = device.DeviceBuffer(hip, 16 * n_tb)
        device.check(hip, hip.svt_hip_txfm_distortion_batch(V(darena.ptr), V(ddesc.ptr), V(ddist.ptr), C.c_uint32(n_tb), C.c_uint32(w),
                                                            C.c_uint32(h), None), "svt_hip_txfm_distortion_batch")
        dist = ddist.download(np.uint64, (n_tb, 2))
    return out, res_raw, dist


def path_run(hip, orc, w, h):
    """The path matrix of one size and the device's answer to it, made once for the tests that read them."""
    if (w, h) not in _RUNS:
        batch = T.path_cases(orc, np.random.default_rng(7000 + w * 100 + h), w, h)
        _RUNS[w, h] = (batch,) + run_fused(hip, w, h, batch, distortion=True)
    return _RUNS[w, h]


def declared(batch, w, h):
    return [o for d in batch["descs"] for o in T.declared_outputs(d, w, h)]


@pytest.mark.parametrize("w,h", T.SIZES)
def test_path_matrix(hip, orc, w, h):
    """Every wave class of tx_cases.CENSUS_CLASSES at every size: coeff, qcoeff, dqcoeff, eob, three_quad_energy, satd, the
    reconstruction and the distortion batch of every block against the oracle."""
    batch, out, res_raw, dist = path_run(hip, orc, w, h)
    T.assert_path_census(orc, w, h, batch)
    T.check_fused_blocks(orc, w, h, batch["descs"], batch["blocks"], out, res_raw, dist, what=(w, h))


@pytest.mark.parametrize("w,h", T.SIZES)
def test_path_matrix_containment(hip, orc, w, h):
    """The same launch wrote nothing but its declared outputs: the inputs, the slack between arrays (a third of the coefficient
    arrays sit 4 / 8 / 12 bytes past a 16-byte boundary) and the columns right of each reconstruction row are untouched."""
    batch, out, _, _ = path_run(hip, orc, w, h)
    check_containment(batch["arena"], out, batch["regions"], declared(batch, w, h), what=(w, h))


@pytest.mark.parametrize("w,h", T.SIZES)
def test_flag_combinations(hip, orc, w, h):
    """tx_cases.FLAG_COMBOS mixed inside the waves of one launch: forward alone (packed and TX_FULLCOEFF), inverse alone from
    dqcoeff_off, the quantiser fed from coeff_off with and without the inverse, TX_SATD against orc_satd over the retained
    block, and a quantiser + inverse with qcoeff_off or dqcoeff_off disabled."""
    batch = T.flag_cases(orc, np.random.default_rng(9000 + w * 100 + h), w, h)
    assert {b["kind"] for b in batch["blocks"]} == set(T.FLAG_COMBOS)
    out, res_raw, _ = run_fused(hip, w, h, batch)
    T.check_fused_blocks(orc, w, h, batch["descs"], batch["blocks"], out, res_raw, what=(w, h))
    check_containment(batch["arena"], out, batch["regions"], declared(batch, w, h), what=(w, h))


@pytest.mark.parametrize("n", [16, 64, 256, 1024])
def test_quantize_batch_paths(hip, orc, n):
    """svt_hip_quantize_batch, 64 blocks per call: all four quantisers, matrices on a third of the blocks, magnitudes up to
    1 << 20 (past the short forms), log_scale 0..2; nothing but qcoeff / dqcoeff is written."""
    batch = T.quantize_batch_cases(orc, np.random.default_rng(500 + n), n)
    arena, darr = batch["arena"], batch["descs"]
    n_tb = len(darr)
    darena = device.DeviceBuffer(hip, arena.nbytes + 256)
    darena.upload(arena)
    ddesc = device.DeviceBuffer(hip, C.sizeof(darr))
    ddesc.upload(np.frombuffer(darr, dtype=np.uint8))
    dres = device.DeviceBuffer(hip, abi.TXFM_RESULT_BYTES * n_tb)
    dres.fill(GUARD)
    device.check(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    device.check(hip, hip.svt_hip_quantize_batch(V(darena.ptr), V(ddesc.ptr), V(dres.ptr), C.c_uint32(n_tb), C.c_uint32(n), None),
                 "svt_hip_quantize_batch")
    out = darena.download(np.uint8, (arena.nbytes,))
    res_raw = dres.download(np.uint8, (n_tb, abi.TXFM_RESULT_BYTES))
    for i, (qc, dq, eob) in enumerate(batch["expect"]):
        d = darr[i]
        assert np.array_equal(out[d.qcoeff_off:d.qcoeff_off + 4 * n].view(np.int32), qc), ("qcoeff", n, i, d.quant_mode)
        assert np.array_equal(out[d.dqcoeff_off:d.dqcoeff_off + 4 * n].view(np.int32), dq), ("dqcoeff", n, i, d.quant_mode)
        r = abi.TxfmResult.from_buffer_copy(res_raw[i].tobytes())
        assert (r.eob, r.three_quad_energy, r.satd) == (eob, 0, 0), ("result", n, i, d.quant_mode)
    check_containment(arena, out, batch["regions"], [(off, 4 * n) for d in darr for off in (d.qcoeff_off, d.dqcoeff_off)], what=n)
