"""The truth of the gather tests: the greedy decomposition of a query signature over reference signatures (include/ntcard_hip.h:
ntc_signature_gather_device) in plain numpy.  Every query entry starts live; a round counts, per reference, the live query entries it holds (np.isin), the
reference with the most wins (np.argmax: the first maximum, so the lowest index among equals), the run stops when that count is below the threshold, when
max_rows rows are written or after len(refs) rounds; else the round reports (ref, common, unique, unique_weight) and the entries stop being live.  All
integers; nothing here is taken from the code under test."""
import numpy as np

ROW_DTYPE = np.dtype([("ref", np.uint32), ("reserved", np.uint32), ("common", np.uint64), ("unique", np.uint64), ("unique_weight", np.uint64)])


def positions(q, r):
    """np.flatnonzero(np.isin(q, r)) for a strictly ascending q and an r without repeats, without np.isin's sort of both lists (1024 references of a few
    hundred entries against a query of 50 000 would spend seconds in it); tests/test_sig_gather_host.py holds the two against each other"""
    at = np.searchsorted(q, r)
    ok = at < q.size
    ok[ok] = q[at[ok]] == r[ok]
    return np.sort(at[ok])


def gather(query, counts, refs, threshold=1, max_rows=None):
    """query: strictly ascending uint64; counts: uint32 per query entry or None (1 each); refs: a list of strictly ascending uint64 arrays (the same array
    object may be listed more than once) -> (rows ROW_DTYPE[n_rows], unassigned, unassigned_weight)"""
    q = np.asarray(query, dtype=np.uint64)
    c = np.ones(q.size, dtype=np.uint64) if counts is None else np.asarray(counts).astype(np.uint64)
    assert c.size == q.size and len(refs) >= 1 and bool(np.all(q[:-1] < q[1:]))
    threshold = max(int(threshold), 1)
    cap = len(refs) if max_rows is None else min(int(max_rows), len(refs))
    # np.isin(q[live], r) per round = (np.isin(q, r) & live): the membership of the whole query is computed once per distinct array
    seen = {}
    member = []
    for r in refs:
        if id(r) not in seen:
            seen[id(r)] = positions(q, np.asarray(r, dtype=np.uint64))
        member.append(seen[id(r)])
    live = np.ones(q.size, dtype=bool)
    rows = []
    every = np.concatenate(member)  # all references' query positions behind one another, and the reference each belongs to
    owner = np.repeat(np.arange(len(refs)), [m.size for m in member])
    for _ in range(len(refs)):
        unique = np.bincount(owner[live[every]], minlength=len(refs))  # per reference: its live query entries
        i = int(np.argmax(unique))
        if unique[i] < threshold or len(rows) >= cap:
            break
        taken = member[i][live[member[i]]]
        rows.append((i, 0, member[i].size, taken.size, int(c[taken].sum(dtype=np.uint64))))
        live[taken] = False
    return np.array(rows, dtype=ROW_DTYPE), int(np.count_nonzero(live)), int(c[live].sum(dtype=np.uint64))


def same(got, want):
    """(rows, unassigned, unassigned_weight) of the device against the model's -> bool"""
    (gr, gu, gw), (wr, wu, ww) = got, want
    return (gr.shape == wr.shape and all(np.array_equal(gr[f].astype(np.uint64), wr[f].astype(np.uint64)) for f in ROW_DTYPE.names)
            and int(gu) == int(wu) and int(gw) == int(ww))
