"""The rule by which k_gc_state derives the mask flags after mode 0's promotion from the flags before it, in numpy.

k_gc_flags ORs one word per pixel: bit 0 FGD, bit 1 BGD, bit 2 a value outside {0, 1, 2, 3}, bit 3 / bit 4 the background /
foreground class (BGD or PR_BGD / FGD or PR_FGD) has a pixel; a bad value belongs to neither class.  k_gc_promote turns an
image's probable label into the definite one exactly when the definite one is absent.  A second flags pass over the
promoted mask therefore gives f2 = f1 | (f1 & 16 ? 1 : 0) | (f1 & 8 ? 2 : 0), which is what k_gc_state computes; this
test checks the rule on every subset of present mask values {0, 1, 2, 3, bad}, and what k_gc_state decides from it."""
import itertools

import numpy as np

BGD, FGD, PR_BGD, PR_FGD, BAD = 0, 1, 2, 3, 7


def flags(mask):
    f = 0
    for m in np.unique(mask):
        if m > 3:
            f |= 4
        else:
            f |= (1 if m == FGD else 0) | (2 if m == BGD else 0) | (8 if m in (BGD, PR_BGD) else 16)
    return f


def promote(mask, f):
    m = mask.copy()
    if not f & 1:
        m[mask == PR_FGD] = FGD
    if not f & 2:
        m[mask == PR_BGD] = BGD
    return m


def derived(f1):
    return f1 | (1 if f1 & 16 else 0) | (2 if f1 & 8 else 0)


def state(f2, mode):
    err = bool(f2 & 4)
    s = err or (mode == 0 and (f2 & 3) != 3) or (mode != 2 and (f2 & 24) != 24)
    return int(s), err


def test_flags_after_promotion_are_a_function_of_the_flags_before():
    values = [BGD, FGD, PR_BGD, PR_FGD, BAD]
    rng = np.random.default_rng(0)
    seen = 0
    for n in range(1, 6):
        for subset in itertools.combinations(values, n):
            mask = np.array(subset * 3, np.uint8)
            rng.shuffle(mask)
            f1 = flags(mask)
            f2 = flags(promote(mask, f1))
            assert derived(f1) == f2, (subset, f1, f2)
            assert state(derived(f1), 0) == state(f2, 0), subset
            # what the set-up must decide: a bad value is an error, a missing class or definite label skips the image
            want_skip = BAD in subset or not ({BGD, PR_BGD} & set(subset)) or not ({FGD, PR_FGD} & set(subset))
            assert state(derived(f1), 0) == (int(want_skip), BAD in subset), subset
            seen += 1
    assert seen == 31


def test_modes_without_promotion_keep_the_flags():
    for subset in ((BGD, PR_FGD), (PR_BGD, PR_FGD), (BGD,), (PR_FGD, BAD)):
        f1 = flags(np.array(subset, np.uint8))
        assert state(f1, 1) == (int(len(subset) < 2 or BAD in subset), BAD in subset)
        assert state(f1, 2)[0] == int(BAD in subset)
