"""The device pass of the feature fuzzer (tests/fuzz_features.py): 40 cases per family at two fixed seeds, every output
array_equal to the family's integer restatement, and all families' cases once more, shuffled, on the one context, so that
consecutive calls alternate between large and small shapes and between entries that share scratch: S_MISC_A between
ggc_apply_hints (clicks) and ggc_seed_from_prior (seed_prior), S_CC_C between ggc_clean_mask (clean) and
ggc_mask_iou (mask_iou), the relax lists between geodesic hints and scissors.  Scratch grows, is reused unzeroed at a
smaller size, and no result may depend on what it held.  Once an entry has given up (a GGCError on valid input, behind
which a fault of the card may stand), the remaining ids fail without touching the GPU.  The long passes are run by hand
(numbers in the fuzzer's header)."""
import numpy as np
import pytest

import fuzz_features as ff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return ff.Device()


@pytest.mark.parametrize("seed", ff.SUITE_SEEDS)
@pytest.mark.parametrize("family", ff.FAMILIES)
def test_family_matches_its_reference(dev, oracle, family, seed):
    assert not ff.GAVE_UP, "an entry gave up earlier on this context: " + ff.GAVE_UP[0]
    lines = ff.run_family(dev, family, seed, oracle)
    assert not lines, "\n" + "\n".join(lines)


@pytest.mark.parametrize("seed", ff.SUITE_SEEDS)
def test_interleaved_families_on_one_context(dev, oracle, seed):
    assert not ff.GAVE_UP, "an entry gave up earlier on this context: " + ff.GAVE_UP[0]
    order = [(family, i) for family in ff.FAMILIES for i in range(ff.N_CASES)]
    np.random.default_rng(1000 + seed).shuffle(order)
    assert len({f for f, _ in order[:20]}) >= 5                         # the families do alternate
    lines = []
    for family, i in order:
        lines += ff.run_case(dev, ff.suite_cases(family, seed)[i], ff.suite_reference(family, seed, i, oracle))
        if lines and ff.REFUSED in lines[-1]:
            break                                                       # an entry gave up: nothing more on this context
    assert not lines, "\n" + "\n".join(lines)
