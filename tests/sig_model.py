"""Model of a signature plane (include/ntcard_hip.h: NTC_FLAG_SIGNATURE): the values an engine hands to ntComp (ntcard.cpp:132-145), those ntComp samples,
and np.unique over them.  Built from the oracle's primitives alone (tests/orc.py, tests/strand_model.py, tests/hpc_model.py): it never sees the code under
test."""
import functools

import numpy as np

import hpc_model as hm
import orc
import strand_model as sm
from support import sampled


def values(reads, spec, strand="canonical"):
    """every value of one plane over the reads; spec: an int k (plain k-mers) or a mask string"""
    if isinstance(spec, int) and strand == "canonical":
        v = [orc.hash_read(r, spec)[0] for r in reads]
        return np.concatenate(v) if v else np.zeros(0, np.uint64)
    mask = "1" * spec if isinstance(spec, int) else spec
    (fs, rs), = sm.values_of(reads, [mask])
    return sm.pick(fs, rs, sm.STRANDS[strand])


def model(reads, spec, strand="canonical", s=7, hpc=False):
    """-> (hashes uint64 ascending, counts int64): the signature of one plane"""
    if hpc:
        reads = hm.model(reads)
    v = values(list(reads), spec, strand)
    h, c = np.unique(v[sampled(v, s)], return_counts=True)
    return h.astype(np.uint64), c.astype(np.int64)


@functools.lru_cache(maxsize=None)
def equal_reads():
    return tuple(sm.sketch_reads_equal())


@functools.lru_cache(maxsize=None)
def equal_model(spec, strand="canonical", s=7, hpc=False):
    """model() over strand_model.sketch_reads_equal(), computed once per configuration and never changed"""
    h, c = model(equal_reads(), spec, strand, s, hpc)
    h.setflags(write=False)
    c.setflags(write=False)
    return h, c
