"""The cover of a reference (kbo_hip.h "The COVER of a reference") on the host: the base offsets, kbo_cover_refset_host - the CPU
restatement of the three kernels over kbo_amd/csrc/refset_cover.hpp - the call without runs, and the argument errors.

The yardstick is brute force written here from the header's definitions, with nothing of the library's walk: the dict of
tests/test_refset_locate_host.py from every k-mer of every indexed stretch of a reference (and of the reverse complements with
add_revcomp) to its occurrences; for every run every window is looked up in it, the canonical occurrence (FWD before REV, then the
smallest p) increments H, and D and every field of the record come from H with numpy.  All comparisons are exact: every field of
every record and every word of the profile.  tools/refset_cover_check.cpp runs the count, the scan and the reduce through accessors
that check every index, as a stand-alone program under AddressSanitizer and UBSan.  No GPU.
tests/test_gpu_refset_cover.py takes the brute force and planted() from here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

from test_refset_locate_host import (ACGT, E_BAD_ARG, E_EMPTY_QUERY, E_LEN_LE_2, REPEAT, SHORT, WIDE, WIDE_ROWS, _rnd, _sub, make_refs, revcomp,
                                     occurrences, strand_seq, world)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NO_ENTRIES, OVERFLOW = 1, 2
NEW_SYMBOLS = ["kbo_refset_cover_bases", "kbo_refset_cover_offsets", "kbo_cover_refset", "kbo_cover_refset_host", "kbo_cover_refset_dev_work_bytes",
               "kbo_cover_refset_dev"]


# ---- brute force
def has_entries(rs, r):
    return rs.status(r) == 0 and rs.route(r) in (refset.ROUTE_LDS, refset.ROUTE_WIDE)


def brute_cover(refs, dicts, entries, k, seqs, runs):
    """(covers, profile, offsets, n_rev) by the definitions: entries[r] says whether reference r has entries; n_rev counts the anchors
    whose canonical occurrence is REV"""
    n = len(refs)
    H = [np.zeros(len(ref), dtype=np.int64) for ref in refs]
    n_runs, n_multi, n_rev = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), 0
    strands = {}
    for w in runs:
        r, s, strand, start, end = int(w["ref"]), int(w["seq"]), int(w["strand"]), int(w["start"]), int(w["end"])
        assert entries[r] and strand in (1, 2) and start <= end <= len(seqs[s])  # usable
        if (s, strand) not in strands:
            strands[s, strand] = strand_seq(seqs[s], strand).tobytes()
        q, d = strands[s, strand], dicts[r]
        n_runs[r] += 1
        for i in range(start, end - k + 1):
            occ = d.get(q[i:i + k])
            if occ is None:
                continue
            rev, p = min(occ)
            H[r][p] += 1
            n_multi[r] += len(occ) > 1
            n_rev += rev
    covers = np.zeros(n, dtype=refset.REF_COVER)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    profile = []
    for r in range(n):
        L = len(refs[r])
        offsets[r + 1] = offsets[r] + (L if entries[r] else 0)
        if not entries[r]:
            covers[r] = (L, 0, 0, NONE, NONE, 0, 0, NO_ENTRIES, 0, 0)
            continue
        c = np.concatenate([[0], np.cumsum(H[r])])
        j = np.arange(L)
        D = c[j + 1] - c[np.maximum(0, j - k + 1)]
        on = D > 0
        at = np.flatnonzero(on)
        begins = on & ~np.concatenate([[False], on[:-1]])
        covers[r] = (L, int(on.sum()), int(begins.sum()), at[0] if len(at) else NONE, at[-1] if len(at) else NONE, int(D.max()) if L else 0,
                     n_runs[r], 0, int(H[r].sum()), n_multi[r])
        profile.append(D.astype(np.uint32))
    return covers, np.concatenate(profile + [np.zeros(0, dtype=np.uint32)]), offsets, n_rev


def assert_same(got, exp, what=""):
    """(covers, profile, offsets) against brute force: every field, every word"""
    covers, profile, offsets = got
    assert np.array_equal(offsets, exp[2]), what
    bad = [r for r in range(len(covers)) if tuple(covers[r]) != tuple(exp[0][r])]
    assert not bad, (what, bad[:5], [(covers[r], exp[0][r]) for r in bad[:3]])
    assert profile.dtype == np.uint32 and np.array_equal(profile, exp[1]), (what, np.flatnonzero(profile != exp[1])[:5])


def assert_identities(k, covers, profile, offsets):
    for r, c in enumerate(covers):
        D = profile[int(offsets[r]):int(offsets[r + 1])]
        assert not c["flags"] & OVERFLOW
        if c["flags"] & NO_ENTRIES:
            assert len(D) == 0 and tuple(c)[1:] == (0, 0, NONE, NONE, 0, 0, NO_ENTRIES, 0, 0)
            continue
        assert len(D) == c["ref_len"] and int(D.sum(dtype=np.uint64)) == k * int(c["n_anchors"])
        assert c["covered"] <= c["ref_len"] and (c["covered"] == 0) == (c["n_anchors"] == 0)
        assert c["covered"] == int((D > 0).sum()) and c["max_depth"] == (int(D.max()) if len(D) else 0) and c["n_multi"] <= c["n_anchors"]
        assert (c["first"] == NONE) == (c["covered"] == 0) == (c["last"] == NONE) == (c["n_segments"] == 0)


def world_entries(w):
    return [has_entries(w.rs, r) for r in range(len(w.refs))]


# ---- planted cases: a set of its own and runs made by hand, one scenario per reference
class Planted:
    def __init__(self, k, rc):
        rng = np.random.default_rng(9100 + k + rc)
        self.k, self.rc = k, rc
        self.refs, self.seqs, runs, self.at = [], [], [], {}

        def ref(name, n):
            self.at[name] = len(self.refs)
            self.refs.append(_rnd(rng, n))
            return self.refs[-1]

        def run(name, seq, strand=1, start=0, end=None, times=1):
            self.seqs.append(np.asarray(seq, dtype=np.uint8))
            runs.extend([(self.at[name], len(self.seqs) - 1, strand, start, len(seq) if end is None else end, 0, 0, 0, 0, 0)] * times)

        self.lengths = sorted({k, k + 1, 64, 65, 63 + k})
        for n in self.lengths:  # (a reference of fewer than k bases has a status: bit 0, and no run may name it)
            a = ref("len%d" % n, n)
            if n >= k:
                run("len%d" % n, a)
        a = ref("ends", 300)              # hit starts at p = 0 and p = L - k, nothing between
        run("ends", a[:k])
        run("ends", a[300 - k:])
        a = ref("adjacent", 300)          # p and p + k: one segment of 2 k bases, over the tile boundary 127|128
        run("adjacent", a[100:100 + k])
        run("adjacent", a[100 + k:100 + 2 * k])
        a = ref("one apart", 300)         # p and p + k + 1: two segments, one uncovered base between them
        run("one apart", a[100:100 + k])
        run("one apart", a[101 + k:101 + 2 * k])
        a = ref("from 64", 300)           # a segment that begins on a tile's first base: 63 uncovered, 64 covered
        run("from 64", a[64:64 + k + 3])
        a = ref("to 127", 300)            # ... and one that ends on a tile's last base
        run("to 127", a[128 - k:128] if k <= 128 else a[:k])
        a = ref("over 63|64", 300)        # a segment that goes on over a tile boundary is not counted again
        run("over 63|64", a[40:40 + k + 30])
        a = ref("repeat", 400)            # an exact repeat: every k-mer of it is MULTI and counts at the first copy only
        a[250:250 + k + 20] = a[50:50 + k + 20]
        run("repeat", a[250:250 + k + 20])
        a = ref("rev", 300)               # the reverse complement of a piece on '+': REV occurrences with add_revcomp, else nothing
        run("rev", revcomp(a[50:50 + k + 5]))
        a = ref("minus", 300)             # ... and read on '-': the piece itself, in the coordinates of the reverse complement
        run("minus", np.concatenate([_rnd(rng, 7), revcomp(a[60:60 + k + 9])]), strand=2, start=0, end=k + 9)
        a = ref("twice", 300)             # the same record twice: the depth doubles
        run("twice", a[200:200 + k + 2], times=2)
        a = ref("short run", 300)         # a run shorter than k
        run("short run", a[10:10 + k + 5], start=2, end=k + 1)
        ref("untouched", 300)
        ref("status", k - 1)
        ref("single index", 20000)
        self.runs = np.array(runs, dtype=refset.REF_RUN)
        self.rs = refset.RefSet.build(self.refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4), positions=True)  # (no wide_rows)
        self.dicts = [occurrences(ref, k, rc) for ref in self.refs]
        self.entries = [has_entries(self.rs, r) for r in range(len(self.refs))]
        self._exp = None

    def expected(self):
        if self._exp is None:
            self._exp = brute_cover(self.refs, self.dicts, self.entries, self.k, self.seqs, self.runs)
        return self._exp

    def assert_reached(self, covers, profile, offsets):
        """every planted case occurs in the records and the profile of a call over self.runs"""
        k, at = self.k, self.at
        D = lambda name: profile[int(offsets[at[name]]):int(offsets[at[name] + 1])]
        rec = lambda name: covers[at[name]]
        reached = {}
        for n in self.lengths:
            c = rec("len%d" % n)
            if n < k:
                reached["len%d" % n] = c["flags"] == NO_ENTRIES and c["ref_len"] == n and self.rs.status(at["len%d" % n]) != 0
            else:
                reached["len%d" % n] = (c["covered"] == n and c["n_segments"] == 1 and (c["first"], c["last"]) == (0, n - 1) and
                                        c["n_anchors"] == n - k + 1 and c["max_depth"] == min(k, n - k + 1) and len(D("len%d" % n)) == n)
        c, d = rec("ends"), D("ends")
        reached["p = 0 and p = L - k"] = (c["first"], c["last"], c["covered"], c["n_segments"], c["n_anchors"]) == (0, 299, 2 * k, 2, 2) and \
            d[0] == d[k - 1] == d[300 - k] == d[299] == 1 and d[k] == d[299 - k] == 0
        c = rec("adjacent")
        reached["p and p + k"] = (c["first"], c["last"], c["covered"], c["n_segments"], c["max_depth"]) == (100, 99 + 2 * k, 2 * k, 1, 1)
        c, d = rec("one apart"), D("one apart")
        reached["p and p + k + 1"] = (c["first"], c["last"], c["covered"], c["n_segments"]) == (100, 100 + 2 * k, 2 * k, 2) and d[100 + k] == 0
        c, d = rec("from 64"), D("from 64")
        reached["63|64"] = d[63] == 0 and d[64] > 0 and (c["first"], c["n_segments"]) == (64, 1)
        c, d = rec("to 127"), D("to 127")
        reached["127|128"] = k > 128 or (d[127] > 0 and d[128] == 0 and (c["last"], c["n_segments"]) == (127, 1))
        c, d = rec("over 63|64"), D("over 63|64")
        reached["over a tile boundary"] = d[63] > 0 and d[64] > 0 and c["n_segments"] == 1 and c["covered"] == k + 30
        reached["j - k crosses a tile"] = k < 64 or rec("over 63|64")["last"] - k >= 0  # (k = 96: S[j - k] lies in another tile for every j)
        c, d = rec("repeat"), D("repeat")
        reached["multi"] = c["n_multi"] == c["n_anchors"] == 21 and (c["first"], c["last"]) == (50, 70 + k - 1) and not d[250:].any()
        c = rec("rev")
        reached["rev"] = (c["n_anchors"], c["covered"], c["first"]) == ((6, k + 5, 50) if self.rc else (0, 0, NONE)) and c["n_runs"] == 1
        c = rec("minus")
        reached["minus"] = (c["n_anchors"], c["covered"], c["first"], c["last"]) == (10, k + 9, 60, 60 + k + 8)
        c, d = rec("twice"), D("twice")
        reached["twice"] = (c["n_runs"], c["n_anchors"], c["covered"], c["max_depth"]) == (2, 6, k + 2, 2 * min(k, 3)) and not (d % 2).any()
        c = rec("short run")
        reached["a run shorter than k"] = (c["n_runs"], c["n_anchors"], c["covered"], c["first"], c["flags"]) == (1, 0, 0, NONE, 0)
        c = rec("untouched")
        reached["untouched"] = tuple(c) == (300, 0, 0, NONE, NONE, 0, 0, 0, 0, 0)
        for name in ("status", "single index"):
            reached[name] = tuple(rec(name)) == (len(self.refs[at[name]]), 0, 0, NONE, NONE, 0, 0, NO_ENTRIES, 0, 0) and len(D(name)) == 0
        missing = [n for n, ok in reached.items() if not ok]
        assert not missing, missing
        assert self.rs.route(at["single index"]) == refset.ROUTE_INDEX and self.rs.status(at["status"]) != 0


_planted = {}


def planted(k, rc):
    if (k, rc) not in _planted:
        _planted[k, rc] = Planted(k, rc)
    return _planted[k, rc]


# ---- the tests
def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, hdr), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"uint64_t n_multi;[^}]*\} kbo_ref_cover;", hdr) and "pub struct RefCover" in rust
    assert "#define KBO_COVER_NO_ENTRIES 1u" in hdr and "#define KBO_COVER_OVERFLOW 2u" in hdr
    assert C.sizeof(_capi.RefCover) == 48 == refset.REF_COVER.itemsize
    assert [refset.REF_COVER.fields[n][1] for n, _ in _capi.RefCover._fields_] == [getattr(_capi.RefCover, n).offset for n, _ in _capi.RefCover._fields_]
    for fn in (refset.cover_refset, refset.cover_refset_dev, kbo_amd.cover_refset, refset.RefSet.cover_offsets, refset.RefSet.cover_bases,
               refset.RefSet.cover_work_bytes):
        assert callable(fn)


def test_the_base_offsets_and_the_work_figure():
    L = kbo_amd.lib()
    w = world(31, False)
    entries = world_entries(w)
    assert entries.count(False) == 1 and not entries[SHORT] and w.rs.route(WIDE) == refset.ROUTE_WIDE
    off = w.rs.cover_offsets()
    assert off[0] == 0 and [int(v) for v in np.diff(off)] == [len(ref) if entries[r] else 0 for r, ref in enumerate(w.refs)]
    assert w.rs.cover_bases() == int(off[-1]) == sum(len(ref) for ref in w.refs) - len(w.refs[SHORT])
    round16 = lambda v: (v + 15) // 16 * 16
    assert w.rs.cover_work_bytes() == round16(24 * len(w.refs)) + round16(4 * int(off[-1]))
    before = w.rs.positions_bytes()
    assert before == 4 * sum(len(w.rs.positions(r)) for r in range(len(w.refs))) + 8 * (len(w.refs) + 1)  # as it was: the offsets are not in it
    plain = refset.RefSet.build(w.refs, kbo_amd.BuildOpts(k=31), wide_rows=WIDE_ROWS)
    out = np.zeros(len(w.refs) + 1, dtype=np.uint64)
    assert plain.cover_bases() == 0 == plain.cover_work_bytes() and L.kbo_refset_cover_offsets(plain._h, out.ctypes.data) == E_BAD_ARG
    assert L.kbo_refset_cover_offsets(w.rs._h, None) == E_BAD_ARG and L.kbo_refset_cover_offsets(None, out.ctypes.data) == E_BAD_ARG
    assert L.kbo_refset_cover_bases(None) == 0 == L.kbo_cover_refset_dev_work_bytes(None)
    # the single-index route owns no base either
    p = planted(31, False)
    off = p.rs.cover_offsets()
    assert [int(v) for v in np.diff(off)] == [len(ref) if p.entries[r] else 0 for r, ref in enumerate(p.refs)]
    assert p.entries.count(False) == 2


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", [31, 96])
def test_cover_host_against_brute_force_over_finds_runs(k, rc):
    """the fixtures of the GPU test on the CPU: find's runs of both strands, of each strand alone, and in another order"""
    w = world(k, rc)
    runs = w.cpu_runs()
    entries = world_entries(w)
    assert len(runs) > 40
    n_rev_seen = 0
    for strands in (3, 1, 2):
        part = runs[(runs["strand"] & strands) != 0]
        assert len(part) > (20 if strands & 1 or rc else 0)
        exp = brute_cover(w.refs, w.dicts, entries, k, w.seqs, part)
        got = refset.cover_refset(w.seqs, w.rs, part, depth=True, host=True)
        assert_same(got, exp, "strands %d" % strands)
        assert_identities(k, *got)
        only = refset.cover_refset(w.seqs, w.rs, part, host=True)  # without the profile: the same records
        assert only.tobytes() == got[0].tobytes()
        n_rev_seen += exp[3]
        if strands == 3:
            c = got[0]
            assert c["n_multi"][REPEAT] > 0 and c["covered"][WIDE] > 0 and c["n_segments"].max() > 1 and c["max_depth"].max() > k
            assert c["flags"][SHORT] == NO_ENTRIES and c["flags"].sum() == NO_ENTRIES and (c["n_runs"] > 0).sum() >= 10
            shuffled = part[np.random.default_rng(k).permutation(len(part))]
            again = refset.cover_refset(w.seqs, w.rs, shuffled, depth=True, host=True)
            assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    assert (n_rev_seen > 0) == rc


@pytest.mark.parametrize("rc", [False, True])
def test_cover_host_at_k_5(rc):
    """4^5 k-mers: every reference is full of repeats, most anchors are MULTI and many occurrences REV"""
    k = 5
    refs = make_refs(k, 300 + k)
    refs = [r[:400] for r in refs[:6]] + [refs[WIDE][:3000], refs[SHORT]]
    rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=2), wide_rows=WIDE_ROWS, positions=True)
    entries = [has_entries(rs, r) for r in range(len(refs))]
    assert entries == [True] * 7 + [False]
    rng = np.random.default_rng(55)
    seqs = [_sub(refs[0][20:300], range(9, 280, 13)), np.concatenate([_rnd(rng, 30), revcomp(refs[3][100:260]), _rnd(rng, 4)]), _rnd(rng, 500),
            refs[6][1000:1700].copy(), refs[1][:k].copy()]
    seqs[3][[100, 350]] = ord("N")
    made = []
    for r in range(7):
        for s, q in enumerate(seqs):
            made += [(r, s, 1, 0, len(q), 0, 0, 0, 0, 0), (r, s, 2, 0, len(q), 0, 0, 0, 0, 0)]
            if len(q) > 70:
                made += [(r, s, 1 + (r + s) % 2, 3, 70, 0, 0, 0, 0, 0), (r, s, 1, 60, 60 + k - 1, 0, 0, 0, 0, 0), (r, s, 2, len(q) - k, len(q), 0, 0, 0, 0, 0)]
    runs = np.array(made, dtype=refset.REF_RUN)
    exp = brute_cover(refs, [occurrences(ref, k, rc) for ref in refs], entries, k, seqs, runs)
    got = refset.cover_refset(seqs, rs, runs, depth=True, host=True)
    assert_same(got, exp)
    assert_identities(k, *got)
    assert (got[0]["n_multi"][:7] > 0).all() and (exp[3] > 0) == rc and got[0]["max_depth"].max() > 2 * k and got[0]["n_segments"].max() > 3


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", [31, 96])
def test_planted_cases(k, rc):
    p = planted(k, rc)
    got = refset.cover_refset(p.seqs, p.rs, p.runs, depth=True, host=True)
    assert_same(got, p.expected())
    assert_identities(k, *got)
    p.assert_reached(*got)
    assert (p.expected()[3] > 0) == rc


def test_a_set_where_no_run_has_an_anchor_and_a_call_without_runs():
    w = world(31, True)
    rng = np.random.default_rng(3)
    seqs = [_rnd(rng, 400), _rnd(rng, 90), _rnd(rng, 31)]
    made = [(r, s, strand, 0, len(q), 0, 0, 0, 0, 0) for r in (0, 5, WIDE) for s, q in enumerate(seqs) for strand in (1, 2)]
    runs = np.array(made, dtype=refset.REF_RUN)
    entries = world_entries(w)
    got = refset.cover_refset(seqs, w.rs, runs, depth=True, host=True)
    assert_same(got, brute_cover(w.refs, w.dicts, entries, 31, seqs, runs))
    c = got[0]
    assert not c["n_anchors"].any() and not c["covered"].any() and not got[1].any() and c["n_runs"].sum() == len(runs)
    assert (c["first"] == NONE).all() and (c["last"] == NONE).all()
    # no runs at all: kbo_cover_refset itself, which then touches no device; the profile is written, not left as it was
    L = kbo_amd.lib()
    concat, off = np.concatenate(seqs), np.array([0, 400, 490, 521], dtype=np.uint64)
    for fn in (L.kbo_cover_refset, L.kbo_cover_refset_host):
        covers = np.full(len(w.refs), 0x77, dtype=np.uint8).repeat(48).view(refset.REF_COVER)
        profile = np.full(w.rs.cover_bases(), 0x77777777, dtype=np.uint32)
        for r_ptr in (None, runs.ctypes.data):
            assert fn(w.rs._h, concat.ctypes.data, off.ctypes.data, 3, r_ptr, 0, covers.ctypes.data, profile.ctypes.data) == 0
            assert not profile.any()
            for r in range(len(w.refs)):
                assert tuple(covers[r]) == (len(w.refs[r]), 0, 0, NONE, NONE, 0, 0, 0 if entries[r] else NO_ENTRIES, 0, 0)
        assert fn(w.rs._h, concat.ctypes.data, off.ctypes.data, 3, None, 0, covers.ctypes.data, None) == 0


def test_argument_errors_and_their_order_need_no_device():
    L = kbo_amd.lib()
    w = world(31, False)
    plain = refset.RefSet.build(w.refs, kbo_amd.BuildOpts(k=31), wide_rows=WIDE_ROWS)
    concat = np.concatenate(w.seqs)
    off = w.offsets.copy()
    good = np.zeros(2, dtype=refset.REF_RUN)
    good["ref"], good["seq"], good["strand"], good["start"], good["end"] = [0, 12], [0, 5], [1, 2], [5, 0], [200, len(w.seqs[5])]
    covers = np.zeros(len(w.refs), dtype=refset.REF_COVER)
    depth = np.zeros(w.rs.cover_bases(), dtype=np.uint32)
    Q, OFF, RUNS, CNT, COVERS, DEPTH, WORK = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000  # device pointers that nothing ever follows

    for fn in (L.kbo_cover_refset_host, L.kbo_cover_refset):
        def call(h=w.rs._h, q=concat.ctypes.data, o=off, n_seqs=len(w.seqs), runs=good, n=None, out=covers.ctypes.data, d=depth.ctypes.data):
            n = len(runs) if n is None and runs is not None else (n or 0)
            return fn(h, q, None if o is None else o.ctypes.data, n_seqs, None if runs is None else runs.ctypes.data, n, out, d)
        if fn is L.kbo_cover_refset_host:
            assert call() == 0 and call(d=None) == 0
        assert call(n=0) == 0 and call(runs=None, n=0, d=None) == 0  # nothing to do: no device is touched
        for kw in (dict(h=None), dict(q=None), dict(o=None), dict(runs=None, n=2), dict(out=None), dict(out=None, n=0)):
            assert call(**kw) == E_BAD_ARG, kw
        assert call(h=plain._h) == E_BAD_ARG and call(h=plain._h, n_seqs=0) == E_BAD_ARG  # no positions: before the batch
        assert call(n_seqs=0) == E_EMPTY_QUERY
        o2 = off.copy()
        o2[2] = o2[1] + 2
        assert call(o=o2) == E_LEN_LE_2
        o2[2] = o2[1] - 1
        assert call(o=o2) == E_BAD_ARG
        o2 = off.copy()
        o2[0] = 1
        assert call(o=o2) == E_BAD_ARG
        # the unusable records, after the batch: an unusable record AND a bad batch reports the batch
        for field, value in (("ref", len(w.refs)), ("ref", SHORT), ("seq", len(w.seqs)), ("strand", 0), ("strand", 3), ("start", 201),
                             ("end", len(w.seqs[0]) + 1), ("ref", 0xFFFFFFFF)):
            bad = good.copy()
            bad[field][0] = value
            assert call(runs=bad) == E_BAD_ARG, (field, value)
            assert call(runs=bad, n_seqs=0) == E_EMPTY_QUERY
        edge = good.copy()
        edge["start"][0] = edge["end"][0] = len(w.seqs[0])  # start == end == len is a run of nothing, not an error
        if fn is L.kbo_cover_refset_host:
            assert call(runs=edge) == 0
    # a run of the single-index route is refused like one of a reference with a status
    p = planted(31, False)
    one = np.zeros(1, dtype=refset.REF_RUN)
    one["ref"], one["strand"], one["end"] = p.at["single index"], 1, 20
    with pytest.raises(kbo_amd.KboError) as e:
        refset.cover_refset(p.seqs, p.rs, one, host=True)
    assert e.value.code == E_BAD_ARG

    # (a set of its own: world()'s sets are shared with the GPU tests, which give them a device copy, and these pointers are fake)
    fresh = refset.RefSet.build(w.refs[:3], kbo_amd.BuildOpts(k=31), positions=True)
    wb = fresh.cover_work_bytes()
    assert wb > 0

    def dev(h=fresh._h, q=Q, o=OFF, n_seqs=6, total=int(off[-1]), runs=RUNS, cnt=CNT, cap=10, out=COVERS, d=DEPTH, work=WORK, work_bytes=wb):
        return L.kbo_cover_refset_dev(h, q, o, n_seqs, total, runs, cnt, cap, out, d, work, work_bytes, None)
    for kw in (dict(h=None), dict(q=None), dict(o=None), dict(cnt=None), dict(runs=None), dict(out=None), dict(work=None), dict(q=Q + 8),
               dict(o=OFF + 4), dict(cnt=CNT + 4), dict(runs=RUNS + 2), dict(out=COVERS + 1), dict(d=DEPTH + 2), dict(work=WORK + 8),
               dict(work_bytes=wb - 1), dict(work_bytes=0), dict(h=plain._h), dict(h=plain._h, n_seqs=0, work_bytes=0)):
        assert dev(**kw) == E_BAD_ARG, kw
    assert dev(n_seqs=0) == E_EMPTY_QUERY and dev(n_seqs=0, work_bytes=0) == E_EMPTY_QUERY  # (the batch before the scratch)
    assert dev() == E_BAD_ARG and dev(d=None) == E_BAD_ARG and dev(runs=None, cap=0) == E_BAD_ARG  # no copy on a device: nothing is enqueued


def test_cover_arithmetic_under_sanitizers(tmp_path):
    """tools/refset_cover_check.cpp: the count, the scan with its tile and carry and the reduce with its tile carries of
    refset_cover.hpp through accessors that check every index, against brute force of its own"""
    exe = str(tmp_path / "refset_cover_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "refset_cover_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "in range" in run.stdout and "agree" in run.stdout
