"""The plan structures a device copy builds for itself and map_reads_kernel then trusts - the 2-bit text in its interleaved and split
forms (pc_tm, pc_t, pc_mu, pc_mc), the device-built seed table and its text positions (seed_tab, seed_pos), the filter in front of
the depth table (dfilt), the anchors (anchor) and the bit per text position that settles a lone substitution (sub_clean) - read back
whole through kbo_index_plan_part (kbo_hip_tuning.h) and compared, EVERY entry, with a numpy restatement of their definitions.

What the restatements are made from is independent of the kernels that wrote the arrays (pack_text_kernel, mark_cells_kernel,
seed_pos_kernel, subst_bits_kernel: map_kernels.hip; dtab_seed_kernel, dtab_filter_kernel, dtab_anchor_kernel: dtab_kernels.hip):
  the contigs themselves          "a suffix of a row" = a string inside an ACGT run of at least k bases (test_gpu_dtab._present's
                                  definition; as a sorted key array here, so that 16 and 17 bases fit)
  Sbwt.path_cover()               text and positions (pinned to the host's construction by kbo_index_cover_check, asserted 0 first)
  the oracle index's rows         spelled with Index.access_kmer, for row intervals and "the suffix of exactly one row"
The depth table is not an input.  Every comparison is exact equality over the whole array; nothing is sampled.

Definitions restated (where each comes from):
  pc_tm / pc_t   map_text.hpp, pack_text_kernel's comment: unit u = positions [16 u - 192, + 16), 2 bits a position, the first one most
                 significant; marks 01 where the position is outside the text or the cover text holds no ACGT byte (its digit is 0
                 there: device_util.hpp pack16 of a zero byte); pc_t[u] == pc_tm[u].x, the 16 bytes behind pc_t read as zero
  pc_mu          map_text.hpp: bit u set iff pc_tm[u].y != 0; every bit from n_units to the array's end and the 4 bytes of slack set
  pc_mc          map_text.hpp cell_marked: bit c set iff ((c + 1) << shift) + 11 > n_units or a unit of [c << shift,
                 ((c + 1) << shift) + 11) has its pc_mu bit set; shift = cell_shift(n_units)
  seed_tab       dtab_seed_kernel's comment: {l, r} = the rows (colex order) whose last seed_d characters spell the string, none of
                 them '$'; absent strings {0, 0}
  seed_pos       seed_pos_kernel: pos[l] | (r - l > 1) << 31, 0xFFFFFFFF for an absent string
  dfilt          dtab_filter_kernel's comment: bit key & 31 of word key >> 5 set iff the string of dfilt_bases bases is a suffix of a row
  sub_clean      map_subst.hpp (a) and (b), for every position of every unit
  anchor         dtab_anchor_kernel / device_util.hpp dtab_anchor_depth: as a SET (slot order depends on atomicCAS races) the slots
                 {((uint32_t)key + 1) << 32 | pos[l]} of the strings of `order` bases that are the suffix of exactly one row, each
                 reachable from (key * 0x9E3779B97F4A7C15) >> (64 - bits) by linear probing without crossing an empty slot

The anchors' tags.  A slot's tag is the low 32 bits of its key (+ 1), so at 17 bases - 34 bits - two strings that differ only in
their oldest base share a tag, and dtab_anchor_depth takes the first slot on its walk of at most 64 slots whose tag matches.  The
property checked for EVERY present string, unique or not: its walk meets its tag on no other key's slot.
  - Up to 16 bases the tag is the whole key: the property cannot fail (it is checked all the same).
  - At 17 bases two keys with one tag differ by d << 32, d = 1 .. 3, and the multiplicative hash puts their home slots a FIXED distance
    apart: (d * 0x7F4A7C15 mod 2^32) >> (32 - bits), give or take one - 0.4972, 0.9945 and 0.4917 of the table.  Only d = 2 (A <-> G,
    C <-> T) comes close: 0.0055 x 2^bits slots.  From 2^14 slots on (about 4 000 rows) that is more than the walk's 64 slots, so on
    the 45 kbp genome (2^17 slots: 727 slots) no pair can meet, whatever is planted; test_tags_of_17_bases asserts that arithmetic
    and runs the planted pair's reads against the oracle anyway.
  - It CAN be built on an index of a few hundred rows (2^9 slots: the homes are two or three slots apart):
    test_two_keys_with_one_tag_on_one_walk plants it, shows from the downloaded table that the walk of the string that is in two
    rows does meet its tag on the other string's slot, and that the answer is still right on every route: dtab_anchor_depth compares the
    text in front of the slot's position with the query from the newest base on, finds the difference at the oldest of the `order`
    bases and answers "unknown" (its `t >= order ? t : kDtabUnknown`), never 16.  The supposition that it prices such a string off
    the wrong row does not hold; these reads are the regression for it.
  - A tag of 0 (sixteen T's at 16 bases) with text position 0 would be an empty slot.  The cover cannot put that row there: position 0
    is the first head in row order, row 0, whose characters are all '$' (asserted); the planted run's slot is found with tag 0.

Each comparator is first shown to bite, on the host: one bit or slot of the downloaded array is changed in numpy and the comparator
must name exactly that entry."""
import os

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, derandomize, synth
from gpu_helpers import threads
from test_gpu_dtab import _present
from test_gpu_map_subst_bits import _genome, _other

pytestmark = pytest.mark.gpu

K = 31
PAD = 192            # positions in front of text position 0 (kernels.hpp kMapPad)
CELLS = 2048         # map_text.hpp kCells
UNITS = 12           # map_text.hpp kUnits
GOLD = np.uint64(0x9E3779B97F4A7C15)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.full(256, 4, dtype=np.int64)
CODE[list(b"ACGT")] = np.arange(4)
TEXT_PARTS = ("pc_tm", "pc_t", "pc_mu", "pc_mc")
ALL_PARTS = TEXT_PARTS + ("seed_tab", "seed_pos", "dfilt", "anchor", "sub_clean")


# ---------------------------------------------------------------------------------------------------------------- the restatements
def _keys(codes, s):
    """key[i] of the s codes from i on (the first one most significant), -1 where one of them is no base"""
    n = len(codes) - s + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    key, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for t in range(s):
        w = codes[t:t + n]
        key = key * 4 + (w & 3)
        bad |= w > 3
    key[bad] = -1
    return key


def _present_keys(contigs, k, s):
    """sorted keys of the strings of s bases inside the ACGT runs of at least k bases: the suffixes of s bases of the index's rows"""
    out = [np.zeros(0, dtype=np.int64)]
    for c in contigs:
        codes = CODE[np.frombuffer(bytes(c), dtype=np.uint8)]
        edges = np.concatenate([[-1], np.flatnonzero(codes > 3), [len(codes)]])
        for a, b in zip(edges[:-1] + 1, edges[1:]):
            if b - a >= max(k, s):
                out.append(_keys(codes[a:b], s))
    return np.unique(np.concatenate(out))


def _isin(keys, sorted_keys):
    if len(sorted_keys) == 0:
        return np.zeros(len(keys), dtype=bool)
    i = np.minimum(np.searchsorted(sorted_keys, keys), len(sorted_keys) - 1)
    return sorted_keys[i] == keys


def _n_units(n_sets):
    return (n_sets + PAD + 256) // 16 + 2  # kernels.hpp pack_text_units


def _ref_text(text, n_units):
    """-> (digit, marked) per position of the padded text, (digits, marks) words per unit"""
    assert set(np.unique(text).tolist()) <= set(b"\0ACGT"), "the cover text holds ACGT and the 0 of a path start"
    assert 16 * n_units >= PAD + len(text)
    byts = np.zeros(16 * n_units, dtype=np.uint8)
    byts[PAD:PAD + len(text)] = text
    code = CODE[byts]
    marked = code > 3
    digit = np.where(marked, 0, code)
    sh = 2 * (15 - np.arange(16, dtype=np.int64))
    digits = (digit.reshape(-1, 16) << sh).sum(axis=1).astype(np.uint32)
    marks = (marked.reshape(-1, 16).astype(np.int64) << sh).sum(axis=1).astype(np.uint32)
    return digit, marked, digits, marks


def _ref_mu(marks, n_units):
    """bytes of pc_mu with its 4 bytes of slack"""
    bits = np.ones((n_units + 255) // 256 * 256 + 32, dtype=bool)
    bits[:n_units] = marks != 0
    return np.packbits(bits, bitorder="little")


def _cell_shift(n_units):
    s = 5
    while (CELLS << s) < n_units:
        s += 1
    return s


def _ref_mc(marks, n_units):
    shift = _cell_shift(n_units)
    seen = np.concatenate([[0], np.cumsum(marks != 0)])
    out = np.zeros(CELLS, dtype=bool)
    for c in range(CELLS):
        lo, hi = c << shift, ((c + 1) << shift) + UNITS - 1
        out[c] = hi > n_units or seen[hi] > seen[lo]
    return np.packbits(out, bitorder="little").view("<u4"), shift, out


def _sub_windows(order, thr, anch):
    """map_subst.hpp window_step / window_used / window_offset -> the offsets of the proof's windows, or None: no bitmap speaks for them"""
    if order < 2 or order > 32 or thr < order or (anch and thr == order):
        return None
    cov = thr - order if anch else thr - order + 2
    if 3 * cov < order - 1:  # window_used(kWindows): a fifth window - not this kernel's
        return None
    return sorted({min(i * cov, order - 1) for i in range(4) if i == 0 or (i - 1) * cov < order - 1})


def _ref_sub_clean(digit, marked, present, order, thr, anch):
    """bool per position q of the padded text: map_subst.hpp's clean()"""
    npos = len(digit)
    out = np.zeros(npos, dtype=bool)
    offs = _sub_windows(order, thr, anch)
    if offs is None:
        return out
    q = np.arange(order - 1, npos - order + 1)  # q + 1 >= order, q + order <= positions
    seen = np.concatenate([[0], np.cumsum(marked)])
    q = q[seen[q + order] == seen[q - order + 1]]  # (a): no mark in [q - (order - 1), q + (order - 1)]
    wkey = _keys(digit, order)
    own, clean = digit[q], np.ones(len(q), dtype=bool)
    for o in offs:  # (b): position q is base o from the window's end
        key = wkey[q + o - order + 1]
        for step in (1, 2, 3):
            alt = (key & ~(3 << (2 * o))) | (((own + step) & 3) << (2 * o))
            clean &= ~_isin(alt, present)
    out[q[clean]] = True
    return out


def _rows(ora):
    """codes (4 for '$') of every row's k characters, rows in colex order"""
    n, k = ora.n_sets, ora.k
    return CODE[np.frombuffer(b"".join(ora.access_kmer(i) for i in range(n)), dtype=np.uint8).reshape(n, k)]


def _row_intervals(rows, s):
    """-> (keys, l, r): the strings of s bases that are the last s characters of a row, and the rows [l, r) that end with each"""
    suf = rows[:, rows.shape[1] - s:]
    idx = np.flatnonzero((suf < 4).all(axis=1))
    key = np.zeros(len(idx), dtype=np.int64)
    for t in range(s):
        key = key * 4 + suf[idx, t]
    keys, first, counts = np.unique(key, return_index=True, return_counts=True)
    assert bool((idx[first + counts - 1] - idx[first] == counts - 1).all()), "rows with one suffix are neighbours in colex order"
    return keys, idx[first], idx[first] + counts


def _hash(keys, bits):
    return ((keys.astype(np.uint64) * GOLD) >> np.uint64(64 - bits)).astype(np.int64)


def _tag(keys):
    return ((keys.astype(np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF))


def _anchor_values(keys, pos_l):
    return (_tag(keys) << np.uint64(32)) | pos_l.astype(np.uint64)


def _anchor_bits(n_rows, order):
    most = n_rows if order >= 16 else min(n_rows, 4 ** order)  # kernels.hpp dtab_anchor_bits
    b = 4
    while (1 << b) < 2 * most + 16:
        b += 1
    return b


# ---------------------------------------------------------------------------------------------------------------- the comparators
def _diff(got, want):
    """entries that differ (the sizes must agree)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "size: got %s, expected %s" % (got.shape, want.shape)
    return np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))


def _assert_same(what, got, want):
    bad = _diff(got, want)
    assert len(bad) == 0, "%s: %d entries differ, first at %d: got %s, expected %s" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def _bit_diff(words, want_bits):
    """-> (positions wrongly set, positions wrongly clear) of a bitmap against a bool per position; bits beyond them must be clear"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)
    assert len(bits) >= len(want_bits)
    want = np.zeros(len(bits), dtype=bool)
    want[:len(want_bits)] = want_bits
    return np.flatnonzero(bits & ~want), np.flatnonzero(~bits & want)


def _assert_bits(what, words, want_bits):
    wrong_set, wrong_clear = _bit_diff(words, want_bits)
    assert len(wrong_set) == 0 and len(wrong_clear) == 0, (
        "%s: %d bits wrongly SET (a wrong character), first %s; %d bits wrongly CLEAR (a lost look-up), first %s" % (
            what, len(wrong_set), wrong_set[:4], len(wrong_clear), wrong_clear[:4]))


def _anchor_report(slots, bits, keys, values, walkers, own):
    """slots: the table; keys / values: the strings that are the suffix of one row and their slots; walkers: every present string,
    own: its slot's value (0: it has none - more than one row).  -> dict of what is wrong:
      missing / extra   values that should be a slot and are none / slots that no string accounts for
      unreachable       keys whose slot lies behind an empty slot of their probe run
      met               walkers whose walk (64 slots at most, up to the first empty one) meets their tag on a slot that is not theirs"""
    size = 1 << bits
    assert len(slots) == size
    nz = slots[slots != 0]
    want = values[values != 0]  # (tag 0 at text position 0 reads as an empty slot: the kernel then answers "unknown")
    rep = {"missing": np.setdiff1d(want, nz), "extra": np.setdiff1d(nz, want), "double": len(nz) - len(np.unique(nz))}
    order_ = np.argsort(slots, kind="stable")
    at = order_[np.minimum(np.searchsorted(slots[order_], values), size - 1)]
    have = (slots[at] == values) & (values != 0)
    empty = np.concatenate([[0], np.cumsum(np.tile(slots == 0, 2))])
    h = _hash(keys, bits)
    idx = np.where(at >= h, at, at + size)
    rep["unreachable"] = keys[have & (empty[idx + 1] != empty[h])]
    hw, tw = _hash(walkers, bits), _tag(walkers)
    win = slots[(hw[:, None] + np.arange(64)) & (size - 1)]
    alive = np.cumprod(win != 0, axis=1).astype(bool)
    hit = alive & ((win >> np.uint64(32)) == tw[:, None])
    first = win[np.arange(len(walkers)), hit.argmax(axis=1)]
    rep["met"] = walkers[hit.any(axis=1) & (first != own)]
    return rep


def _assert_anchor(what, rep, allow_met=()):
    met = np.setdiff1d(rep["met"], np.asarray(allow_met, dtype=np.int64))
    assert len(rep["missing"]) == 0 and len(rep["extra"]) == 0 and rep["double"] == 0 and len(rep["unreachable"]) == 0 and len(met) == 0, (
        "%s: %d slots missing (first %s), %d slots of no string (first %s), %d slots twice, %d keys behind an empty slot (first %s), "
        "%d strings whose walk meets their tag on another key's slot (first %s)" % (
            what, len(rep["missing"]), rep["missing"][:2], len(rep["extra"]), rep["extra"][:2], rep["double"], len(rep["unreachable"]),
            rep["unreachable"][:2], len(met), met[:2]))


# ---------------------------------------------------------------------------------------------------------------- copies and worlds
def _copy(contigs, k=K, order=0, anchors=-1, seed_d=0, env=None):
    """an index and its device copy with its plan structures, made at once under these knobs (restored whatever happens)"""
    L = kbo_amd.lib()
    L.kbo_set_plan_lazy(0)
    L.kbo_set_depth_table(order)
    L.kbo_set_depth_table_anchors(anchors)
    L.kbo_set_seed_table_depth(seed_d)
    for name, value in (env or {}).items():
        os.environ[name] = value
    try:
        sbwt, _ = kbo_amd.build([bytes(c) for c in contigs], kbo_amd.BuildOpts(k=k, num_threads=threads()))
        sbwt.to_device(-1)
        sbwt.plan_part("pc_tm")  # (whatever makes the plan structures makes them here, under this environment)
    finally:
        for name in (env or {}):
            os.environ.pop(name, None)
        L.kbo_set_plan_lazy(-1)
        L.kbo_set_depth_table(0)
        L.kbo_set_depth_table_anchors(-1)
        L.kbo_set_seed_table_depth(0)
    return sbwt


def _cover(sbwt):
    """path_cover(), after kbo_index_cover_check says it is the host's construction"""
    import ctypes as C
    d = C.c_uint64(1)
    kbo_amd.check(kbo_amd.lib().kbo_index_cover_check(sbwt._h, C.byref(d)))
    assert d.value == 0, "the copy's path cover differs from the host's construction at %d entries" % d.value
    return sbwt.path_cover()


def _threshold(sbwt, k):
    return int(derandomize.random_match_threshold(k, sbwt.n_kmers(), 4, 1e-7)) if sbwt.n_kmers() else 0


class World:
    """an index copy, the inputs of the restatements, and the restated text"""

    def __init__(self, contigs, sbwt, k=K, ora=None):
        self.contigs, self.sbwt, self.k, self.ora = contigs, sbwt, k, ora
        self.text, self.pos, self.node = _cover(sbwt)
        self.n_units = _n_units(sbwt.n_sets())
        self.digit, self.marked, self.digits, self.marks = _ref_text(self.text, self.n_units)
        self.rows = _rows(ora) if ora is not None else None
        if ora is not None:
            assert ora.n_sets == sbwt.n_sets()
        self._present = {}

    def present(self, s):
        if s not in self._present:
            self._present[s] = _present_keys(self.contigs, self.k, s)
            if self.rows is not None:  # (the two references agree on what a suffix of a row is)
                assert np.array_equal(_row_intervals(self.rows, s)[0], self._present[s])
        return self._present[s]

    def part(self, name):
        return self.sbwt.plan_part(name)


def _check_text_parts(w, what):
    n = w.n_units
    tm, info = w.part("pc_tm")
    assert info[0] == n and info[1] == _cell_shift(n) and tm.shape == (n, 2), (what, info, tm.shape)
    _assert_same(what + ": pc_tm", tm, np.stack([w.digits, w.marks], axis=1))
    t, info = w.part("pc_t")
    assert info[:2] == [n, _cell_shift(n)] and len(t) == n + 4, (what, info, len(t))  # (the 16 bytes a window's last load may read)
    _assert_same(what + ": pc_t", t, np.concatenate([w.digits, np.zeros(4, dtype=np.uint32)]))
    mu, info = w.part("pc_mu")
    want_mu = _ref_mu(w.marks, n)
    assert info[:2] == [n, _cell_shift(n)] and len(mu) == (n + 255) // 256 * 32 + 4, (what, info, len(mu))
    _assert_same(what + ": pc_mu", mu, want_mu)
    mc, info = w.part("pc_mc")
    want_mc, shift, cells = _ref_mc(w.marks, n)
    assert info[:2] == [n, shift] and len(mc) == CELLS // 32, (what, info, len(mc))
    _assert_same(what + ": pc_mc", mc, want_mc)
    return tm, t, mu, mc, cells


def _sub_rule(w, order, anchors_there):
    """device_index.cpp: the threshold of a call with default options, whether the proof runs with anchors, and whether the copy has a
    bitmap at all (a threshold the table's order reaches, below k, a proof of at most four windows)"""
    thr = _threshold(w.sbwt, w.k)
    anch = anchors_there and thr > order
    has = thr >= order and thr < w.k and thr > 0 and _sub_windows(order, thr, anch) is not None
    return thr, anch, has


def _check_sub_clean(w, what, order, anchors_there):
    """-> (words, the reference's bool per position) or (None, None) where the rule gives the copy no bitmap"""
    thr, anch, has = _sub_rule(w, order, anchors_there)
    words, info = w.part("sub_clean")
    if not has:
        assert len(words) == 0, "%s: a bitmap of %d words where the rule gives none (thr %d, order %d)" % (what, len(words), thr, order)
        return None, None
    assert len(words) == (w.n_units + 1) // 2, "%s: %d words, bitmap_words says %d" % (what, len(words), (w.n_units + 1) // 2)
    assert info == [w.n_units, order, thr, int(anch)], (what, info, thr, anch)
    want = _ref_sub_clean(w.digit, w.marked, w.present(order), order, thr, anch)
    _assert_bits(what + ": sub_clean", words, want)
    return words, want


def _anchor_inputs(w, order):
    keys, l, r = _row_intervals(w.rows, order)
    one = r - l == 1
    values = _anchor_values(keys[one], w.pos[l[one]])
    own = np.zeros(len(keys), dtype=np.uint64)
    own[one] = values
    return keys, one, values, own


def _check_anchor(w, what, order, allow_met=()):
    slots, info = w.part("anchor")
    bits = _anchor_bits(w.sbwt.n_sets(), order)
    assert info[:2] == [bits, order] and len(slots) == 1 << bits, (what, info, len(slots))
    keys, one, values, own = _anchor_inputs(w, order)
    assert np.array_equal(keys, w.present(order))
    rep = _anchor_report(slots, bits, keys[one], values, keys, own)
    _assert_anchor(what + ": anchor", rep, allow_met)
    return slots, bits, keys, one, values, own, rep


def _agree(w, reads, what):
    """the reads through matches_batch (map_reads_kernel, or the kernel for sequences of any length where one has more than 160 bases)
    and ms_batch against the oracle, every byte"""
    concat = np.concatenate(reads)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    chars, d = w.ora.matches_batch(concat, offsets, 1e-7, n_threads=threads(), want_d=True)
    kbo_amd.lib().kbo_set_plan(1, 0, 0)
    got = batch.matches_batch(w.sbwt, concat, offsets)
    lens = np.diff(offsets.astype(np.int64))
    keep = np.repeat(lens >= 3, lens)  # (the characters of sequences of fewer than 3 bases are unspecified)
    bad = np.flatnonzero((got != chars) & keep)
    assert len(bad) == 0, "%s, matches_batch: %d characters differ, first at byte %d" % (what, len(bad), bad[0])
    for _ in range(2):  # (a launch that gave the plan up holds the next one off: both must be exact)
        ms, _, _ = batch.ms_batch(w.sbwt, concat, offsets)
        bad = np.flatnonzero(ms != d)
        assert len(bad) == 0, "%s, ms_batch: %d values differ, first at byte %d: %d, expected %d" % (what, len(bad), bad[0], ms[bad[0]], d[bad[0]])


# ---------------------------------------------------------------------------------------------------------------- 1, 2: every part
def _twelve_short():
    rng = np.random.default_rng(8_2027)
    return [synth.genome(int(n), seed=700 + i) for i, n in enumerate(rng.integers(300, 501, 12))]


@pytest.fixture(scope="module")
def near_copies(oracle):
    g = _genome()
    return World([g], _copy([g]), ora=oracle.Index.build([g.tobytes()], k=K))


@pytest.fixture(scope="module")
def many_starts(oracle):
    contigs = _twelve_short() + [_genome()]
    return World(contigs, _copy(contigs), ora=oracle.Index.build([c.tobytes() for c in contigs], k=K))


def test_near_copies_every_part(near_copies):
    """the 45 kbp genome with planted near-copies, default order and anchors: all nine parts, every entry; then every comparator bites"""
    w = near_copies
    order = w.sbwt.depth_table_order()
    assert order == 11 and w.sbwt.device_layout()["anchor_bytes"] > 0
    tm, t, mu, mc, cells = _check_text_parts(w, "near copies")
    assert int(w.marked[PAD:PAD + len(w.text)].sum()) >= 1  # (path starts: the contig's, and where the near-copies branch)

    # ---- seed_tab, seed_pos
    tab, info = w.part("seed_tab")
    seed_d = info[0]
    assert 4 <= seed_d <= order and info[1] == 1 and tab.shape == (4 ** seed_d, 2), (info, tab.shape)
    keys, l, r = _row_intervals(w.rows, seed_d)
    assert np.array_equal(keys, w.present(seed_d))
    want_tab = np.zeros((4 ** seed_d, 2), dtype=np.uint32)
    want_tab[keys, 0], want_tab[keys, 1] = l, r
    _assert_same("seed_tab", tab, want_tab)
    sp, info = w.part("seed_pos")
    assert info[:2] == [seed_d, 1] and len(sp) == 4 ** seed_d
    want_sp = np.full(4 ** seed_d, 0xFFFFFFFF, dtype=np.uint32)
    want_sp[keys] = w.pos[l] | ((r - l > 1).astype(np.uint32) << 31)
    _assert_same("seed_pos", sp, want_sp)
    # (where no mark lies in the seed_d positions ending there, the cover text at that position spells the string)
    p = w.pos[l].astype(np.int64) + PAD
    seen = np.concatenate([[0], np.cumsum(w.marked)])
    whole = seen[p + 1] == seen[p + 1 - seed_d]
    assert int(whole.sum()) > len(keys) // 2
    assert np.array_equal(_keys(w.digit, seed_d)[p[whole] + 1 - seed_d], keys[whole])
    # ... and the host-built table of a copy without a depth table, at the same depth, wherever a string is present
    host_tab, host_info = _copy(w.contigs, order=-1, seed_d=seed_d).plan_part("seed_tab")
    assert host_info[:2] == [seed_d, 0] and host_tab.shape == tab.shape
    there = host_tab[:, 0] < host_tab[:, 1]
    assert np.array_equal(np.flatnonzero(there), keys) and np.array_equal(host_tab[there], tab[there])

    # ---- dfilt (the brute-force table of test_gpu_dtab._present as the reference)
    filt, info = w.part("dfilt")
    fb = info[0]
    assert 6 <= fb <= order - 2 and info[1] == order and len(filt) == 4 ** fb // 32, (info, len(filt))
    want_f = _present([c.tobytes() for c in w.contigs], K, fb)
    assert 0 < int(want_f.sum()) < len(want_f)
    wrong_set, wrong_clear = _bit_diff(filt, want_f)
    assert len(wrong_set) == 0 and len(wrong_clear) == 0, "dfilt: wrongly set %s, wrongly clear %s" % (wrong_set[:4], wrong_clear[:4])

    # ---- sub_clean: clean and dirty positions both exist, from the reference alone
    words, want = _check_sub_clean(w, "near copies", order, True)
    inner = want[PAD + 400:PAD + len(w.text) - 400]
    assert words is not None and 0 < int(inner.sum()) < len(inner), "the genome has no dirty or no clean position"

    # ---- anchor
    slots, bits, akeys, one, values, own, rep = _check_anchor(w, "near copies", order)
    assert 0 < int((~one).sum()) < len(one)  # (the near-copies: strings that are in two rows)

    # ---- the comparators bite (numpy only): one entry changed, exactly that entry named
    for name, got, ref_, i, bit in (("pc_tm digits", tm, np.stack([w.digits, w.marks], axis=1), 777, 1 << 9), ("pc_t", t, None, len(t) - 1, 1),
                                    ("pc_mu", mu, _ref_mu(w.marks, w.n_units), len(mu) - 1, 0x80), ("pc_mc", mc, _ref_mc(w.marks, w.n_units)[0], 40, 1 << 5),
                                    ("seed_pos", sp, want_sp, int(keys[5]), 1 << 31)):
        ref_ = np.concatenate([w.digits, np.zeros(4, dtype=np.uint32)]) if ref_ is None else ref_
        bad = got.copy()
        at_i = (i, 0) if bad.ndim == 2 else i
        bad[at_i] = bad[at_i] ^ bad.dtype.type(bit)
        assert _diff(bad, ref_).tolist() == [i], name
    bad = tab.copy()
    bad[int(keys[7]), 1] += 1
    assert _diff(bad, want_tab).tolist() == [int(keys[7])]
    q_clean, q_dirty = int(np.flatnonzero(want)[100]), PAD + 400 + int(np.flatnonzero(~inner)[3])
    for q, kind in ((q_clean, 1), (q_dirty, 0)):
        bad = words.copy()
        bad[q >> 5] ^= np.uint32(1 << (q & 31))
        ws, wc = _bit_diff(bad, want)
        assert (ws.tolist(), wc.tolist()) == (([], [q]) if kind else ([q], []))
    key_there, key_absent = int(np.flatnonzero(want_f)[11]), int(np.flatnonzero(~want_f)[11])
    for key, kind in ((key_there, 1), (key_absent, 0)):
        bad = filt.copy()
        bad[key >> 5] ^= np.uint32(1 << (key & 31))
        ws, wc = _bit_diff(bad, want_f)
        assert (ws.tolist(), wc.tolist()) == (([], [key]) if kind else ([key], []))
    # the anchors: a slot emptied is missing; a slot that takes the tag of the key one slot behind it is met on that key's walk
    ukeys = akeys[one]
    order_ = np.argsort(slots, kind="stable")
    at = order_[np.searchsorted(slots[order_], values)]
    bad = slots.copy()
    bad[at[3]] = 0
    rep = _anchor_report(bad, bits, ukeys, values, akeys, own)
    assert rep["missing"].tolist() == [values[3]] and len(rep["extra"]) == 0
    pushed = np.flatnonzero((at == ((_hash(ukeys, bits) + 1) & ((1 << bits) - 1))) & (at > 0))  # keys that sit one slot behind their home
    assert len(pushed) > 0
    j = int(pushed[0])
    bad = slots.copy()
    bad[at[j] - 1] = (values[j] & np.uint64(0xFFFFFFFF00000000)) | (slots[at[j] - 1] & np.uint64(0xFFFFFFFF))
    rep = _anchor_report(bad, bits, ukeys, values, akeys, own)
    assert rep["met"].tolist() == [int(ukeys[j])] and len(rep["missing"]) == 1 and len(rep["extra"]) == 1


def test_many_path_starts_text_parts_and_sub_clean(many_starts):
    """12 contigs of 300 - 500 bases and the 45 kbp one: 13 path starts inside the text; the text parts and sub_clean, every entry"""
    w = many_starts
    order = w.sbwt.depth_table_order()
    _check_text_parts(w, "many path starts")
    assert int(w.marked[PAD:PAD + len(w.text)].sum()) >= 13
    words, want = _check_sub_clean(w, "many path starts", order, w.sbwt.device_layout()["anchor_bytes"] > 0)
    assert words is not None and 0 < int(want.sum())
    starts = np.flatnonzero(w.marked[PAD:PAD + len(w.text)]) + PAD
    for s in starts:  # (a window around a position within order - 1 bases of a path start reaches the mark: not clean)
        assert not want[max(s - order + 1, 0):s + order].any()


# ---------------------------------------------------------------------------------------------------------------- 3: coarse cells
COARSE_RESIDUES = (10, 11, 12, 0, 63, 10, 11, 12, 63, 0, 10, 11, 12, 10, 11, 12)  # unit mod 64 of the path starts behind the first
COARSE_IN_UNIT = (0, 15, 7, 0, 15, 3)                                              # ... and their place in the unit, in turn


def _coarse_first_pass():
    contigs = [synth.genome(1_060_000, seed=4242)] + [synth.genome(4_400, seed=9_000 + i) for i in range(len(COARSE_RESIDUES))]
    sbwt, _ = kbo_amd.build([c.tobytes() for c in contigs], kbo_amd.BuildOpts(k=K, num_threads=threads()))
    text = sbwt.path_cover()[0]
    starts = np.flatnonzero(text == 0)
    assert len(starts) == len(contigs) and starts[0] == 0
    last = {c[-K:].tobytes(): i for i, c in enumerate(contigs)}
    bounds = np.concatenate([starts, [len(text)]])
    chain = [last[text[b - K:b].tobytes()] for b in bounds[1:]]  # the contig whose bases end each path
    assert sorted(chain) == list(range(len(contigs)))
    return contigs, starts, chain, len(text)


def _coarse_contigs(first_pass, units_mod_256):
    """Every path of the first pass's cover ends with one contig's last bases, so a contig cut short at its end by d bases moves every
    later path start d positions down and nothing else: the cuts that put the path starts into the units COARSE_RESIDUES of their
    cells, and the last one that makes n_units % 256 what the variant asks for."""
    contigs, starts, chain, n = first_pass
    cut, shift = {}, 0
    for i in range(1, len(starts)):
        want = 16 * COARSE_RESIDUES[i - 1] + COARSE_IN_UNIT[i % len(COARSE_IN_UNIT)]
        d = (int(starts[i]) - shift + PAD - want) % 1024  # 64 units of 16 positions: a cell
        cut[chain[i - 1]] = d
        shift += d
    n -= shift
    d = next(d for d in range(4096) if _n_units(n - d) % 256 == units_mod_256)
    cut[chain[-1]] = d
    return [c[:len(c) - cut.get(i, 0)] for i, c in enumerate(contigs)]


@pytest.fixture(scope="module")
def coarse_first_pass():
    return _coarse_first_pass()


@pytest.mark.parametrize("units_mod_256", [1, 255])
def test_coarse_cells_and_the_ballot_writers_edges(coarse_first_pass, units_mod_256):
    """1.1 Mbp: cells of 64 units (cell_shift 6, the smallest size above the minimum), path starts in the units ((c + 1) << 6) + 10,
    + 11 and + 12 - the last unit a window that starts in cell c can see, and the two behind it - of at least three cells each and in a
    cell's first and last unit, n_units % 256 = 1 and 255 (the last wave and the last workgroup of pack_text_kernel's and
    subst_bits_kernel's ballots).  The text parts with their slack, and sub_clean; the conditions asserted from path_cover()."""
    contigs = _coarse_contigs(coarse_first_pass, units_mod_256)
    w = World(contigs, _copy(contigs))
    n = w.n_units
    assert n > 65_536 and _cell_shift(n) == 6 and n % 256 == units_mod_256, n
    starts = np.flatnonzero(w.text == 0)
    assert len(starts) == len(contigs)
    unit = (starts + PAD) >> 4
    for res in (10, 11, 12):
        assert len({int(u) >> 6 for u in unit if u >= 64 and u % 64 == res}) >= 3, (res, unit)
    assert (unit % 64 == 0).any() and (unit % 64 == 63).any(), unit
    tm, t, mu, mc, cells = _check_text_parts(w, "coarse cells")
    used = (n - UNITS + 1) >> 6  # cells whose windows end inside the text
    assert 0 < int(cells[:used].sum()) < used and cells[used:].all()
    for u in unit[1:]:  # the border itself, from the reference: a start in unit ((c + 1) << 6) + 10 is in sight of cell c, one in + 11 is not
        c = (int(u) >> 6) - 1
        if u % 64 == 10:
            assert cells[c]
        if u % 64 in (11, 12):
            assert not cells[c] or ((unit >= (c << 6)) & (unit < ((c + 1) << 6) + 11)).any()
    assert not t[n:].any() and (mu[(n + 255) // 256 * 32:] == 0xFF).all()  # the slack, as downloaded
    order = w.sbwt.depth_table_order()
    words, want = _check_sub_clean(w, "coarse cells", order, w.sbwt.device_layout()["anchor_bytes"] > 0)
    assert words is not None and len(words) == (n + 1) // 2
    # the ballot writers' edges: the last words of the bitmap are written (clean positions exist there: the text ends 16 - 32 units
    # in front of the last unit, so look at the last word that holds any)
    last_word = int(np.flatnonzero(want)[-1]) >> 5
    assert last_word >= len(words) - 24 and words[last_word] != 0
    assert int(want.sum()) > len(w.text) // 2


# ---------------------------------------------------------------------------------------------------------------- 4: orders 16 and 17
T_RUN = 15_000


def _planted_genome():
    """the 45 kbp genome with a run of sixteen T's between two other bases, once"""
    g = _genome()
    g[T_RUN:T_RUN + 16] = ord("T")  # (between the genome's planted near-copies)
    g[T_RUN - 1], g[T_RUN + 16] = ord("G"), ord("C")
    return g


@pytest.mark.parametrize("anchors", [1, 0], ids=["anchors", "no_anchors"])
def test_order_16_and_a_tag_of_zero(oracle, anchors):
    """16 bases (the kernels' 64-bit keys begin above): the anchors with the one string whose tag wraps to 0, and sub_clean where the
    rule gives the copy one (without anchors; with them the proof at this threshold has more windows than the kernel takes)"""
    g = _planted_genome()
    w = World([g], _copy([g], order=16, anchors=anchors), ora=oracle.Index.build([g.tobytes()], k=K))
    assert w.sbwt.depth_table_order() == 16
    words, want = _check_sub_clean(w, "order 16", 16, anchors == 1)
    assert (words is not None) == (anchors == 0)
    if not anchors:
        assert len(w.part("anchor")[0]) == 0
        assert 0 < int(want.sum())
        return
    slots, bits, keys, one, values, own, rep = _check_anchor(w, "order 16", 16)
    t16 = 4 ** 16 - 1
    i = int(np.searchsorted(keys, t16))
    assert keys[i] == t16 and one[i], "sixteen T's are the suffix of exactly one row"
    assert 0 < int(own[i]) < 2 ** 32 and int(own[i]) in set(slots.tolist()), "its slot: tag 0, a text position that is not 0"
    # tag 0 AT text position 0 - an "empty" slot - cannot be: position 0 holds the first head in row order, row 0, all '$'
    assert int(w.node[0]) == 0 and w.ora.access_kmer(0) == b"$" * K
    rng = np.random.default_rng(16)
    reads = []
    for ext in range(5, 21):  # the run behind a substitution, 5 - 20 matching bases in front of it
        r = g[T_RUN - ext - 41:T_RUN - ext - 41 + 150].copy()
        r[40] = _other(r[40], 1 + ext % 3)
        reads.append(r)
    reads += [g[a:a + 150].copy() for a in rng.integers(T_RUN - 200, T_RUN, 8)]
    _agree(w, reads, "order 16")


def _same_tag_distances(bits):
    """slots between the homes of two keys of 34 bits that share their low 32: (d << 32) * GOLD >> (64 - bits), d = 1 .. 3, as the
    shorter way round the table (give or take one slot, by the carry of the low bits)"""
    size = 1 << bits
    out = []
    for d in (1, 2, 3):
        x = ((d * (int(GOLD) & 0xFFFFFFFF)) & 0xFFFFFFFF) >> (32 - bits)
        out.append(min(x, size - x))
    return out


def _pair_reads(contigs, at, k_len, rng, read_len=150):
    """reads that run into the planted string behind a substitution with 5 - 20 matching bases in front of it, and over it whole;
    at: (contig, offset) of every planted string"""
    reads = []
    for ci, p in at:
        c = contigs[ci]
        for ext in range(5, 21):
            a = max(p - ext - 41, 0)
            r = c[a:a + read_len].copy()
            m = p - ext - 1 - a
            if 0 <= m < len(r):
                r[m] = _other(r[m], 1 + ext % 3)
            reads.append(r)
        reads.append(c[max(p - 60, 0):p + k_len + 60].copy())
    return reads


def test_tags_of_17_bases(oracle):
    """17 bases with anchors on the 45 kbp genome, K planted twice and K' = K with its oldest base two codes on planted once: the
    anchors and the rule for sub_clean read back, the pair's reads on every route against the oracle - and the arithmetic that says why
    no walk over 2^17 slots can hold both (this module's docstring)."""
    g = _genome()
    rng = np.random.default_rng(17)
    kmer = ACGT[rng.integers(0, 4, 17)]
    other = kmer.copy()
    other[0] = ACGT[(int(np.searchsorted(ACGT, kmer[0])) + 2) % 4]
    at = [(0, 8_000), (0, 22_000), (0, 15_000)]  # (between the genome's planted near-copies)
    g[8_000:8_017], g[22_000:22_017], g[15_000:15_017] = kmer, kmer, other
    w = World([g], _copy([g], order=17, anchors=1), ora=oracle.Index.build([g.tobytes()], k=K))
    assert w.sbwt.depth_table_order() == 17
    words, _ = _check_sub_clean(w, "order 17", 17, True)
    assert words is None  # (at this threshold the proof with anchors has more than four windows: no bitmap)
    slots, bits, keys, one, values, own, rep = _check_anchor(w, "order 17", 17)
    key_k, key_o = int(_keys(CODE[kmer], 17)[0]), int(_keys(CODE[other], 17)[0])
    assert (key_k ^ key_o) == 2 << 32 and _tag(np.array([key_k]))[0] == _tag(np.array([key_o]))[0]
    i, j = int(np.searchsorted(keys, key_k)), int(np.searchsorted(keys, key_o))
    assert keys[i] == key_k and not one[i] and keys[j] == key_o and one[j], "K is in two rows, K' in one"
    # why the two cannot meet here: their homes are 727 slots apart, every pair's at least that, the walk is 64 slots
    assert bits == 17 and min(_same_tag_distances(bits)) > 64 + 1, _same_tag_distances(bits)
    hk, ho = int(_hash(np.array([key_k]), bits)[0]), int(_hash(np.array([key_o]), bits)[0])
    assert abs(min((hk - ho) % (1 << bits), (ho - hk) % (1 << bits)) - _same_tag_distances(bits)[1]) <= 1
    assert [b for b in range(4, 33) if min(_same_tag_distances(b)) <= 64 + 1] == list(range(4, 14)), "from 2^14 slots on no walk holds two keys of one tag"
    reads = _pair_reads([g], at, 17, rng)
    long_ = [g[p - 300:p + 300].copy() for _, p in at]  # more than 160 bases: the kernel for sequences of any length
    for r in long_:
        r[rng.integers(0, 600, 6)] = ord("A")
    _agree(w, reads, "order 17, reads")
    _agree(w, long_, "order 17, long sequences")


TINY_K = 20


def _tiny_contigs(seed):
    rng = np.random.default_rng(seed)
    kmer = ACGT[rng.integers(0, 4, 17)]
    other = kmer.copy()
    other[0] = ACGT[(int(np.searchsorted(ACGT, kmer[0])) + 2) % 4]
    flank = [ACGT[rng.integers(0, 4, 25)] for _ in range(6)]
    return [np.concatenate([flank[0], kmer, flank[1]]), np.concatenate([flank[2], kmer, flank[3]]), np.concatenate([flank[4], other, flank[5]])], kmer, other


def _tiny_world_model(oracle, seed):
    """-> (contigs, K's key, K''s key, bits) if, by a model of the table (which slots are taken does not depend on the order the keys
    arrive in), K's walk runs over taken slots up to K''s home, which lies 0 - 2 slots behind its own; else None"""
    contigs, kmer, other = _tiny_contigs(seed)
    ora = oracle.Index.build([c.tobytes() for c in contigs], k=TINY_K)
    keys, l, r = _row_intervals(_rows(ora), 17)
    key_k, key_o = int(_keys(CODE[kmer], 17)[0]), int(_keys(CODE[other], 17)[0])
    cnt = dict(zip(keys.tolist(), (r - l).tolist()))
    if cnt.get(key_k) != 2 or cnt.get(key_o) != 1:
        return None
    bits = _anchor_bits(ora.n_sets, 17)
    size = 1 << bits
    taken = set()
    for h in _hash(keys[r - l == 1], bits).tolist():
        while h in taken:
            h = (h + 1) % size
        taken.add(h)
    hk, ho = int(_hash(np.array([key_k]), bits)[0]), int(_hash(np.array([key_o]), bits)[0])
    gap = (ho - hk) % size
    if gap > 2 or any((hk + t) % size not in taken for t in range(gap + 1)):
        return None
    return contigs, key_k, key_o, bits


def test_two_keys_with_one_tag_on_one_walk(oracle):
    """k = 20, three contigs of 67 bases, a table of 17 bases with anchors: small enough (2^9 slots) for K (in two rows: no slot) to
    walk over the slot of K' (one row), which carries K's tag.  Shown from the downloaded table; the text in front of that slot's
    position spells K', so dtab_anchor_depth's comparison fails at the oldest of the 17 bases and it answers "unknown" - the reads
    that extend K by 5 - 20 bases get the oracle's values on every route."""
    found = next((m for m in (_tiny_world_model(oracle, seed) for seed in range(400)) if m is not None), None)
    assert found is not None, "no seed of 400 puts K' on K's walk"
    contigs, key_k, key_o, bits = found
    w = World(contigs, _copy(contigs, k=TINY_K, order=17, anchors=1), k=TINY_K, ora=oracle.Index.build([c.tobytes() for c in contigs], k=TINY_K))
    assert w.sbwt.depth_table_order() == 17 and _anchor_bits(w.sbwt.n_sets(), 17) == bits
    slots, bits, keys, one, values, own, rep = _check_anchor(w, "one tag, one walk", 17, allow_met=[key_k])
    assert rep["met"].tolist() == [key_k], "K's walk meets its tag on the slot of K' - the case this world is built for"
    # what the kernel finds there: the position of K''s row, and in front of it K' - not K - in the cover text
    slot = int(own[int(np.searchsorted(keys, key_o))])
    p = (slot & 0xFFFFFFFF) + PAD
    assert not w.marked[p - 16:p + 1].any() and int(_keys(w.digit, 17)[p - 16]) == key_o != key_k
    rng = np.random.default_rng(3)
    reads = _pair_reads(contigs, [(0, 25), (1, 25), (2, 25)], 17, rng, read_len=67) + [c.copy() for c in contigs]
    _agree(w, reads, "one tag, one walk")
    # ... and as one long sequence (the kernel for sequences of any length)
    _agree(w, [np.concatenate([contigs[0], contigs[2], contigs[1], contigs[0][20:]])], "one tag, one walk, long")


# ---------------------------------------------------------------------------------------------------------------- 5: no bitmap, no table
def _sizes(sbwt):
    return {name: len(sbwt.plan_part(name)[0]) for name in ALL_PARTS}


def test_copies_without_a_bitmap_or_a_table():
    g = _genome()
    n = _sizes(_copy([g], env={"KBO_SUBST_BITS": "0"}))
    assert n["sub_clean"] == 0 and all(n[p] > 0 for p in ALL_PARTS if p != "sub_clean"), n
    # a default threshold below the table's order: 10 k-mers, a table one base above their threshold
    small = synth.genome(40, seed=5)
    thr = int(derandomize.random_match_threshold(K, 10, 4, 1e-7))
    assert thr + 1 <= 17
    sbwt = _copy([small], order=thr + 1)
    assert sbwt.n_kmers() == 10 and sbwt.depth_table_order() == thr + 1
    n = _sizes(sbwt)
    assert n["sub_clean"] == 0 and n["pc_tm"] > 0 and n["pc_t"] > 0, n
    # an index without a k-mer
    sbwt = _copy([synth.genome(20, seed=6)])
    assert sbwt.n_kmers() == 0
    assert _sizes(sbwt)["sub_clean"] == 0
    # no depth table: nothing but the host-built seed table
    sbwt = _copy([g], order=-1)
    n = _sizes(sbwt)
    assert n["seed_tab"] > 0 and sbwt.plan_part("seed_tab")[1][1] == 0 and all(n[p] == 0 for p in ALL_PARTS if p != "seed_tab"), n
