"""ggc_slic_enforce_connectivity against the CPU oracle on small label maps built around the replay of small components:
runs across the 64-pixel wave boundary, one-pixel-wide images, blocks just under min_size that merge along long chains,
blocks that are all carved, and a one-pixel-wide serpentine whose length straddles min_size (a BFS front that turns
corners, and a component queue filled to its last slot).  The last test runs some of the maps with a min_size of several
thousand pixels, where every component of the map is replayed and absorbed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 10 ** 6


def _enforce(gpu_ctx, raw, mn, mx):
    from gcn_grabcut import _native
    raw = np.ascontiguousarray(raw, dtype=np.int32)
    b, h, w = raw.shape
    d = torch.as_tensor(raw).cuda()
    out = torch.empty(b, h, w, dtype=torch.int32, device="cuda")
    n = torch.empty(b, dtype=torch.int32, device="cuda")
    gpu_ctx.call("ggc_slic_enforce_connectivity", _native.current_stream(0), b, h, w, d.data_ptr(), int(mn), int(mx),
                 out.data_ptr(), n.data_ptr())
    return out.cpu().numpy(), n.cpu().numpy()


def _check(oracle, gpu_ctx, raw, mn, mx):
    got, n = _enforce(gpu_ctx, raw, mn, mx)
    for i in range(raw.shape[0]):
        want, wn = oracle.slic_connectivity(raw[i], mn, mx)
        assert np.array_equal(got[i], want), (i, raw.shape, mn, mx, int((got[i] != want).sum()))
        assert n[i] == wn


def _noise(b, h, w, seed):
    return np.random.default_rng(seed).integers(0, 3, (b, h, w)).astype(np.int32)


def _speckled_blocks(b, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = ((yy // 9) * 2 + (xx // 11) * 3) % 5                    # 9 x 11 blocks, 4-neighbours always differ
    raw = np.repeat(base[None], b, axis=0).astype(np.int32)
    speck = rng.random((b, h, w)) < 0.08
    raw[speck] = 5 + rng.integers(0, 3, int(speck.sum()))
    return raw


def _serpentine(h, w, length):
    """A one-pixel-wide path of `length` pixels of label 1 that snakes through a sea of label 0."""
    raw = np.zeros((h, w), np.int32)
    y, x, step, left = 1, 1, 1, length
    while left:
        assert y < h - 1, "map too small for the path"
        raw[y, x] = 1
        left -= 1
        if 1 <= x + step <= w - 2:
            x += step
        else:                                                       # turn: two pixels down, then back
            if left:
                raw[y + 1, x] = 1
                left -= 1
            y += 2
            step = -step
    return raw


@pytest.mark.parametrize("w", [63, 64, 65, 129])
def test_noise_runs_across_the_wave_boundary(oracle, gpu_ctx, w):
    _check(oracle, gpu_ctx, _noise(4, 21, w, seed=w), 6, 40)


@pytest.mark.parametrize("h,w", [(1, 200), (200, 1)])
def test_one_pixel_wide_images(oracle, gpu_ctx, h, w):
    _check(oracle, gpu_ctx, _noise(3, h, w, seed=h), 6, 40)


@pytest.mark.parametrize("mn,mx", [(100, 300), (20, 90)])
def test_speckled_blocks(oracle, gpu_ctx, mn, mx):
    _check(oracle, gpu_ctx, _speckled_blocks(3, 70, 140, seed=mn), mn, mx)


@pytest.mark.parametrize("mn", [100, 400])
def test_serpentine_straddles_min_size(oracle, gpu_ctx, mn):
    h, w = 48, 40
    lengths = [mn - 1, mn, mn + 1]
    raw = np.stack([_serpentine(h, w, n) for n in lengths])
    for i, n in enumerate(lengths):
        assert int((raw[i] == 1).sum()) == n
        want, wn = oracle.slic_connectivity(raw[i], mn, BIG)
        path = want[raw[i] == 1]
        if n < mn:
            assert wn == 1 and (path == 0).all()                    # absorbed by the sea
        else:
            assert wn == 2 and (path == 1).all()                    # keeps a label of its own
    _check(oracle, gpu_ctx, raw, mn, BIG)


def test_min_size_of_thousands_of_pixels(oracle, gpu_ctx):
    _check(oracle, gpu_ctx, _noise(4, 21, 65, seed=7), 5000, BIG)
    _check(oracle, gpu_ctx, _noise(3, 200, 1, seed=8), 5000, BIG)
    _check(oracle, gpu_ctx, _speckled_blocks(3, 70, 140, seed=9), 5000, BIG)
    _check(oracle, gpu_ctx, _speckled_blocks(3, 70, 140, seed=10), 2000, 6000)
