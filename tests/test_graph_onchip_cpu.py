"""The one ordering argument the on-chip region graph rests on, restated in numpy: the pair lists sorted ascending by
key lo*Nmax+hi, adjacent pairs before non-local ones, are the dense matrix's row-major walk of its upper triangle, and a
pair's place in that walk is its row's offset plus the number of the row's entries below it (how k_topology ranks a pair
through the adjacency bitset)."""
import numpy as np
import pytest

NL_BIT = 1 << 30


def dense_walk(m, n):
    """What k_rowcount / k_rowscan / k_extract emit: per row i, the entries j > i in ascending j; adjacent, then non-local."""
    adj, nl = [], []
    for i in range(n):
        for j in range(i + 1, n):
            v = int(m[i, j])
            if v & ~NL_BIT:
                adj.append((i, j, v & ~NL_BIT))
            if v & NL_BIT:
                nl.append((i, j, 0))
    return adj + nl


def sorted_lists(m, n, nmax, rng):
    """The same pairs found in any order (a hash table's), then ordered by key alone."""
    ii, jj = np.nonzero(np.triu(m[:n, :n], 1))
    order = rng.permutation(len(ii))
    ii, jj = ii[order], jj[order]
    v = m[ii, jj]
    key = ii * nmax + jj
    a, s = (v & ~NL_BIT) != 0, (v & NL_BIT) != 0
    ka, kn = np.sort(key[a]), np.sort(key[s])
    cnt = {int(k): int(c & ~NL_BIT) for k, c in zip(key, v)}
    return [(int(k) // nmax, int(k) % nmax, cnt[int(k)]) for k in ka] + [(int(k) // nmax, int(k) % nmax, 0) for k in kn]


def random_dense(rng, n, nmax, fill, empty_rows):
    m = np.zeros((nmax, nmax), np.int64)
    up = np.triu(rng.random((n, n)) < fill, 1)
    m[:n, :n] = np.where(up, rng.integers(1, 500, (n, n)), 0)
    m[:n, :n] |= np.where(np.triu(rng.random((n, n)) < fill / 2, 1), NL_BIT, 0)
    for r in empty_rows:
        if r < n:
            m[r, :] = 0
    return m


@pytest.mark.parametrize("n,nmax,fill,empty_rows", [(1, 1, 0.5, ()), (1, 9, 0.5, ()), (2, 2, 1.0, ()), (7, 7, 0.0, ()),
                                                    (40, 40, 0.05, (0, 5, 39)), (40, 64, 0.3, (1, 2, 3)),
                                                    (129, 200, 0.02, (64, 128)), (64, 64, 1.0, ())])
def test_sorted_keys_are_the_dense_row_major_walk(n, nmax, fill, empty_rows):
    rng = np.random.default_rng(n * 1000 + nmax)
    m = random_dense(rng, n, nmax, fill, empty_rows)
    assert sorted_lists(m, n, nmax, rng) == dense_walk(m, n)


@pytest.mark.parametrize("n,fill", [(1, 0.5), (5, 1.0), (70, 0.1), (33, 0.5)])
def test_rank_is_row_offset_plus_row_bits_below(n, fill):
    rng = np.random.default_rng(n)
    bits = np.triu(rng.random((n, n)) < fill, 1)
    bits = bits | bits.T                                            # the symmetric bitset the k-NN reads
    row_cnt = np.array([np.count_nonzero(bits[i, i + 1:]) for i in range(n)], np.int64)
    off = np.concatenate([[0], np.cumsum(row_cnt)[:-1]]) if n else row_cnt
    keys = sorted(i * n + j for i in range(n) for j in range(i + 1, n) if bits[i, j])
    for i in range(n):
        for j in range(i + 1, n):
            if bits[i, j]:
                assert keys[off[i] + np.count_nonzero(bits[i, i + 1:j])] == i * n + j
    assert len(keys) == row_cnt.sum()
