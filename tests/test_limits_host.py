"""CPU tests of what the limit tests on the GPU rely on (tests/limits_model.py): the directed reads are where they are said to be at every length, the
vectorised forward-strand model is tests/strand_model.py's, the model of the cut's table search finds every entry in the steps the GPU tests assert."""
import numpy as np
import pytest

import limits_model as lm
import orc
import strand_model as sm


@pytest.mark.parametrize("L", [1009, 4097, 32769, 65520, 65535])
@pytest.mark.parametrize("k", [12, 32])
def test_directed_reads_are_present(L, k):
    arr = lm.directed_batch(np.random.default_rng(L + k), 70, L, k)
    assert arr.shape == (70, L) and arr.dtype == np.uint8
    lm.assert_directed(arr, k)
    assert len(lm.DIRECTED) == 9
    windows = L - k + 1
    f1 = [int(orc.sketch_reads([arr[i].tobytes()], [k], 0, 10, 7)[1][0]) for i in range(9)]
    assert f1[0] == f1[8] == f1[6] == windows  # clean; lower case and U; the slot byte is a base to the reference
    assert f1[1] == windows - 1 and f1[2] == windows - 1  # an N on the first / last base costs one window
    assert f1[3] == windows - k and f1[4] == windows - k  # an N on the first base of the last window / one in front of it costs k windows
    s = min(lm.run_centre(L) - 20, L - 40)
    assert f1[7] == windows - (min(s + 39, L - k) - max(s - k + 1, 0) + 1)  # the windows that hold a byte of the run
    with pytest.raises(AssertionError):
        arr[3, L - k] = ord("A")
        lm.assert_directed(arr, k)


def test_tile_array_is_the_package_layout():
    import ntcard_amd as nt
    rng = np.random.default_rng(3)
    for n, L in ((1, 1009), (70, 4097), (2049, 33)):
        arr = lm.random_reads(rng, n, L, 0.01)
        assert np.array_equal(lm.tile_array(arr), nt.tile_reads([arr[i].tobytes() for i in range(n)], L))


@pytest.mark.parametrize("k", [12, 32])
def test_forward_model_is_the_strand_model(k):
    rng = np.random.default_rng(k)
    arr = lm.random_reads(rng, 12, 300, 0.01)
    arr[0, 100] = 1       # the reference's table slots are bases
    arr[1, 7] = 3
    arr[2, :] = ord("N")  # no window at all
    arr[3] = np.frombuffer(b"acgtuACGTU", dtype=np.uint8)[rng.integers(0, 10, size=300)]
    reads = [arr[i].tobytes() for i in range(12)]
    want = np.concatenate([sm.window_values(r, "1" * k)[0] for r in reads])
    assert np.array_equal(lm.forward_values(arr, k), want) and want.size > 2000
    tc, f1 = lm.forward_sketch(arr, k, 10, 3)
    wtc, wf1 = sm.model_sketch(reads, ["1" * k], sm.FORWARD, 10, 3)
    assert np.array_equal(f1, wf1) and np.array_equal(tc, wtc) and tc.any()


def test_blocks_of_a_read():
    assert lm.k1h_blocks(32, 150) == 10 and lm.k1h_blocks(32, 160) == 11  # (test_k1h_emulator.py: a virtual chunk behind the read)
    assert lm.k1h_blocks(12, 65535) == 4097 and lm.k1h_blocks(32, 65535) == 4096 and lm.k1h_blocks(17, 65520) == 4096


def test_table_search_model_finds_every_entry():
    for n in (1, 2, 63, 64, 65, 127, 4096, 4097):
        steps = [lm.cut_search_steps(n, t) for t in range(n)]
        assert max(steps) == {1: 0, 2: 1, 63: 1, 64: 1, 65: 2, 127: 2, 4096: 2, 4097: 3}[n], n
