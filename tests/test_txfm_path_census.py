"""CPU: the inputs of tests/test_gpu_txfm_paths.py reach every quantiser path of the fused transform kernel (their design,
checked where no GPU is needed)."""
import numpy as np
import pytest

import tx_cases as T
from arena import check_containment


@pytest.mark.parametrize("w,h", T.SIZES)
def test_path_cases_census(orc, w, h):
    """tx_cases.path_census states, wave by wave, which of quant_small<true> / quant_small<false> / quant_one the kernel
    chooses for the blocks of tx_cases.path_cases and why.  It mirrors the kernel's wave mapping and path predicate
    (csrc/txfm.hip txfm_kernel, csrc/txfm_block.hpp txfm_block) and must follow them if they change."""
    batch = T.path_cases(orc, np.random.default_rng(7000 + w * 100 + h), w, h)
    T.assert_path_census(orc, w, h, batch)
    # what no descriptor declares as an output covers all inputs and all slack: the containment check has something to guard
    declared = sum(nb for d in batch["descs"] for _, nb in T.declared_outputs(d, w, h))
    assert 0 < declared < batch["arena"].size
    check_containment(batch["arena"], batch["arena"].copy(), batch["regions"], [])
    spoilt = batch["arena"].copy()
    d = batch["descs"][1]
    spoilt[d.recon_off + w * (2 if d.bit_depth != 8 else 1)] ^= 1            # first byte right of row 0 of a reconstruction
    with pytest.raises(AssertionError, match="recon of block 1"):
        check_containment(batch["arena"], spoilt, batch["regions"], [o for x in batch["descs"] for o in T.declared_outputs(x, w, h)])
