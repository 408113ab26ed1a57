"""The three kinds of Bloom filter as siblings (ntcard_amd/bloom.py: BloomFilter, BlockedBloomFilter and CountingBloomFilter under one private base):
`merge` refuses a filter of another kind in Python, before any library call — an image of another layout, or of another length, never reaches the
device — and the blocked kind has the base's save / load under both of its names.  m_bits = 512 is a size every kind takes."""
import itertools

import numpy as np
import pytest

from gpu_support import nt  # noqa: F401  (nt: the fixture)
from ntcard_amd import bloom

pytestmark = pytest.mark.gpu

M, H, K = 512, 3, 32
KINDS = ("BloomFilter", "BlockedBloomFilter", "CountingBloomFilter")


def filled(nt, kind, seed):
    """a filter of the kind with 40 values inserted"""
    f = getattr(nt, kind)(M, H, K)
    f.insert_hashes(np.random.default_rng(seed).integers(0, 1 << 63, size=40, dtype=np.uint64))
    return f


def image(f):
    """the whole device array, padding included"""
    return f.filter.cpu().numpy().copy()


@pytest.mark.parametrize("a_kind,b_kind", list(itertools.permutations(KINDS, 2)), ids=lambda kind: kind)
def test_merge_refuses_another_kind(nt, a_kind, b_kind):
    a, b = filled(nt, a_kind, 1), filled(nt, b_kind, 2)
    assert (a.m_bits, a.n_hash, a.k, a.strand) == (b.m_bits, b.n_hash, b.k, b.strand)  # the shape check alone would let it through
    before, n_before = image(a), a.n_inserted
    with pytest.raises(ValueError):
        a.merge(b)
    assert np.array_equal(image(a), before) and a.n_inserted == n_before


@pytest.mark.parametrize("kind", KINDS)
def test_merge_of_the_same_kind_and_shape(nt, kind):
    a, b = filled(nt, kind, 1), filled(nt, kind, 2)
    ia, ib = image(a), image(b)
    a.merge(b)
    want = np.minimum(ia.astype(np.uint16) + ib, 255).astype(np.uint8) if kind == "CountingBloomFilter" else ia | ib
    assert np.array_equal(image(a), want) and not np.array_equal(want, ia) and a.n_inserted == 80
    with pytest.raises(ValueError):
        a.merge(getattr(nt, kind)(M, H, K + 1))


def test_blocked_save_load_are_write_read(nt, tmp_path):
    f = filled(nt, "BlockedBloomFilter", 3)
    f.save(tmp_path / "saved.bbf")
    f.write(tmp_path / "written.bbf")
    assert (tmp_path / "saved.bbf").read_bytes() == (tmp_path / "written.bbf").read_bytes()
    for back in (nt.BlockedBloomFilter.load(tmp_path / "saved.bbf"), nt.BlockedBloomFilter.read(tmp_path / "saved.bbf")):
        assert type(back) is nt.BlockedBloomFilter
        assert (back.m_bits, back.n_hash, back.k, back.strand, back.n_inserted, back.n_blocks) == (M, H, K, "canonical", 40, 1)
        assert np.array_equal(image(back), image(f))
    header, img = bloom.read_blocked_file(tmp_path / "saved.bbf")
    assert header == {"k": K, "n_hash": H, "strand": "canonical", "m_bits": M, "n_inserted": 40, "block_bits": 512}
    assert np.array_equal(img, f.bytes())


def test_the_kinds_are_siblings(nt):
    """CountingBloomFilter.solid takes `isinstance(into, BloomFilter)` for "a plain filter": a blocked filter must not be one"""
    kinds = [getattr(nt, kind) for kind in KINDS]
    for a, b in itertools.permutations(kinds, 2):
        assert not issubclass(a, b)
    f = filled(nt, "CountingBloomFilter", 4)
    with pytest.raises(ValueError):
        f.solid(None, None, 1, nt.BlockedBloomFilter(M, H, K))
