"""Indel events and sites (kbo_indels_dev, kbo_indel_sites_dev; indel_kernels.hip, index_indel.hpp) at the sizes where their device code
takes another setting than tests/test_gpu_index_indel.py reaches: the carried `run` of sums_scan in all three of its uses, every pass
count of the sort with the result in either key buffer, more keys than one block of the scan under a radix pass, every sorted key
bit, a packed head sum over more than 256 chunks, and the depth rule with 64-bit products and events at both ends of the sources.

The inputs are synthetic arrays uploaded to the device, made with numpy, every device buffer at exactly its documented figure between
guard bands and the inputs asserted unchanged.  What is expected is stated twice: the bytes of the host forms
(kbo_indels_from_segments_host, kbo_indel_sites_host), and a vectorised numpy statement of the header's definitions written here
(vector_events, vector_sites), which agrees with brute_events / brute_sites of tests/test_index_indel_host.py on a prefix or a sample of
a few thousand - nothing expected rests on the library alone.  Every threshold below names the launch line it comes from, and every
test first asserts that its input lies beyond it.

Not covered: twelve passes of the sort need 2^24 source bases; lists of more than 2^30 events."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import locate

from test_gpu_index_indel import CHUNK, T_ALL, TILE, _Lists, _located, _two_segment_reads, _Uploaded
from test_gpu_index_locate import _build
from test_gpu_index_scale import big_handle
from test_index_indel_host import INS, LEN_MASK, LONG, brute_events, brute_sites, event_tuples, host_lists, site_tuples
from test_index_locate_host import ACGT

pytestmark = pytest.mark.gpu

# sums_scan (indel_kernels.hip): ONE workgroup takes the chunks' sums kThreads = 256 at a time, `c0 += kThreads`, a chunk kScanChunk =
# 2048 records, places or groups: `run` is carried beyond 256 * 2048 of them (event_sums_kernel, sums64_kernel, site_sums_kernel)
SCAN_ROUND = 256
SCAN_TURN = SCAN_ROUND * CHUNK
# launch_build_radix_pass (build_kernels.hip): launch_scan(d_hist, 256 * tiles, ...) takes a second block of kScanBlock = 1024 histogram
# words beyond 4 tiles of kBuildTile = 4096 keys
RADIX_SCAN_TURN = 1024 // 256 * TILE
# launch_indel_sites: `for (end = kSortEndBit; end > first;)`, digits of 8 bits from bit 96 down to sort_first_bit(source_bases)
SORT_END_BIT, DIGIT = 96, 8
CODE_LEN = 16
K = 31


def pos_bits(n_bases):
    """index_indel.hpp pos_bits(): the bits a pos <= source_bases can set"""
    return int(n_bases).bit_length()


def sort_passes(n_bases):
    """index_indel.hpp sort_passes(): (kSortEndBit - sort_first_bit + 7) / 8 with sort_first_bit = 32 - pos_bits -> (passes, bits of the top digit)"""
    bits = SORT_END_BIT - (32 - pos_bits(n_bases))
    return (bits + DIGIT - 1) // DIGIT, bits - (bits - 1) // DIGIT * DIGIT


def source_of(soff, x):
    """the last source that begins at or in front of x: an empty source in front of x is passed over"""
    return np.searchsorted(np.asarray(soff[:-1]).astype(np.int64), x, side="right") - 1


# ---- the header's definitions, vectorised
def vector_events(recs, cat, off, k, soff, skip_multi, max_indel):
    """(events in list order, complex junctions) of one call's records from index_indel.hpp's rule, every pair at once"""
    n_seqs, total, bases = len(off) - 1, len(cat), int(soff[-1])
    f = {n: recs[n].astype(np.int64) for n in recs.dtype.names}
    ok_seq = f["seq"] < n_seqs
    s = np.where(ok_seq, f["seq"], 0)
    o, e = off[s].astype(np.int64), off[s + 1].astype(np.int64)
    holds = ok_seq & (f["q_first"] <= f["q_last"]) & (o <= e) & (e <= total) & (f["q_last"] + k <= e - o)
    if skip_multi:
        holds &= (f["flags"] & 12) == 0
    rev = f["flags"] & 1
    s_lo = np.where(rev == 1, f["pos_last"], f["pos_first"])
    s_hi = np.where(rev == 1, f["pos_first"], f["pos_last"]) + k
    A, B = slice(0, -1), slice(1, None)
    pair = holds[A] & holds[B] & (f["seq"][A] == f["seq"][B]) & (rev[A] == rev[B]) & (f["q_last"][A] < f["q_first"][B])
    r = rev[A] == 1
    up_lo = np.where(r, s_lo[A], s_lo[B])
    low_hi = np.where(r, s_hi[B], s_hi[A])
    gq = f["q_first"][B] - (f["q_last"][A] + k)
    gs = up_lo - low_hi
    shift = gs - gq
    near = pair & (shift != 0) & (np.abs(shift) <= min(int(max_indel), LEN_MASK))
    cx = near & (gq > 0) & (gs > 0)
    cand = near & ~cx
    ins = shift < 0
    ln = np.abs(shift)
    pos = np.where(ins, up_lo, up_lo - ln)
    cand &= (pos >= 0) & (up_lo <= bases) & (source_of(soff, up_lo) == source_of(soff, low_hi - 1))
    # an insertion's bytes: FWD [B.q_first - len, B.q_first), REV the reverse complement of [A.q_last + k, A.q_last + k + len)
    at = np.where(r, f["q_last"][A] + k, f["q_first"][B] - ln)
    cand &= ~ins | np.where(r, at + ln <= (e - o)[A], at >= 0)
    code = np.zeros(len(cand), dtype=np.int64)
    x = np.flatnonzero(cand & ins)
    assert not len(x) or ln[x].max() <= 64, "the statement gathers up to 64 bases"
    base = np.full(256, 4, dtype=np.int64)
    base[ACGT] = np.arange(4)
    good = np.ones(len(x), dtype=bool)
    for i in range(int(ln[x].max()) if len(x) else 0):  # i: ascending source order
        live = i < ln[x]
        j = o[A][x] + at[x] + np.where(r[x], ln[x] - 1 - i, i)
        b = base[cat[np.where(live, j, 0)]]
        good &= ~live | (b < 4)
        b = np.where(r[x], 3 - b, b) & 3
        code[x] |= np.where(live & (ln[x] <= CODE_LEN), b << (2 * min(i, CODE_LEN - 1)), 0)
    cand[x[~good]] = False
    w = np.flatnonzero(cand)
    ev = np.zeros(len(w), dtype=locate.INDEL_EVENT_DTYPE)
    ev["pos"] = pos[w]
    ev["kind_len"] = ln[w] | np.where(ins[w], INS | np.where(ln[w] > CODE_LEN, LONG, 0), 0)
    ev["code"] = code[w]
    ev["flags"] = (r[w] != (f["strand"][B][w] == 2)).astype(np.int64)
    return ev, int(cx.sum()), w + 1  # (w + 1: the record a pair ends at)


def events_hold(ev, bases):
    """event_key(): the words hold an event pair_event() writes"""
    pos, kl, code, fl = (ev[n].astype(np.int64) for n in ("pos", "kind_len", "code", "flags"))
    ln, ins, lng = kl & LEN_MASK, (kl & INS) != 0, (kl & LONG) != 0
    ok_ins = (lng == (ln > CODE_LEN)) & ~(lng & (code != 0)) & ~((ln < CODE_LEN) & ((code >> np.minimum(2 * ln, 62)) != 0))
    ok_del = ~lng & (code == 0) & (pos + ln <= bases)
    return (fl <= 1) & (ln > 0) & (pos <= bases) & np.where(ins, ok_ins, ok_del)


def vector_groups(ev, bases):
    """np.unique over the (pos, kind_len, code) of the events that hold one -> (keys [groups, 3] ascending, counts, MINUS bits): the
    (pos, kind_len) words ranked first, so that a rank and a code fit one 64-bit word whose order is the keys'"""
    ok = events_hold(ev, bases)
    w0 = ev["pos"][ok].astype(np.uint64) << np.uint64(32) | ev["kind_len"][ok].astype(np.uint64)
    ranked, rank = np.unique(w0, return_inverse=True)
    uk, inv, cnt = np.unique(rank.astype(np.uint64) << np.uint64(32) | ev["code"][ok].astype(np.uint64), return_inverse=True, return_counts=True)
    w0 = ranked[(uk >> np.uint64(32)).astype(np.int64)]
    u = np.stack([w0 >> np.uint64(32), w0 & np.uint64(0xFFFFFFFF), uk & np.uint64(0xFFFFFFFF)], axis=1).astype(np.int64)
    return u, cnt, np.bincount(inv.ravel(), weights=ev["flags"][ok], minlength=len(u)).astype(np.int64)


def vector_sites(ev, depth, soff, min_count, num, den, groups=None):
    """the sites of a list as INDEL_SITE_DTYPE: the groups' counts against the depth of the base in front, the products in 64 bits"""
    bases = int(soff[-1])
    u, cnt, minus = vector_groups(ev, bases) if groups is None else groups
    d = depth[np.maximum(u[:, 0] - 1, 0)].astype(np.uint64) if bases else np.zeros(len(u), dtype=np.uint64)
    call = (cnt >= min_count) & (cnt.astype(np.uint64) * np.uint64(den) >= np.uint64(num) * d)
    out = np.zeros(int(call.sum()), dtype=locate.INDEL_SITE_DTYPE)
    out["pos"], out["kind_len"], out["code"] = u[call, 0], u[call, 1], u[call, 2]
    out["source"], out["count"], out["n_minus"], out["depth"] = source_of(soff, u[call, 0]), cnt[call], minus[call], d[call]
    return out, u, cnt


def _differ(got, want):
    """for a failure's message: the first records that differ, or the two lengths"""
    if len(got) != len(want):
        return "%d records for %d" % (len(got), len(want))
    words = got.dtype.itemsize // 4
    return np.flatnonzero((got.view(np.uint32).reshape(-1, words) != want.view(np.uint32).reshape(-1, words)).any(axis=1))[:8]


def _events(rows):
    ev = np.zeros(len(rows), dtype=locate.INDEL_EVENT_DTYPE)
    ev["pos"], ev["kind_len"], ev["code"], ev["flags"] = (np.array([r[i] for r in rows], dtype=np.uint32) for i in range(4))
    return ev


def _sites_on_device(sbwt, ev, n_events, depth, ecap, scap, t, stream, seed=1):
    """kbo_indel_sites_dev over an uploaded list -> (sites written, the full count); guard bands and the read-only inputs checked"""
    import torch
    p = _Lists(sbwt, 0, ecap, scap, seed=seed, events=ev, n_events=n_events, depth=depth)
    torch.cuda.synchronize()
    p.finish(t, stream, depth=False)
    torch.cuda.synchronize()
    _, ne, sites, ns = p.results("event capacity %d, site capacity %d, thresholds %s" % (ecap, scap, (t,)))
    assert ne == n_events and not p.events.changed() and not p.depth.changed() and not p.ecnt.changed(), "the list, its count and d_depth are read only"
    return sites, ns


# ---- 1. the event scan over more than one round of the sums
READS = ("insertion", "deletion", "hp_del", "hp_ins", "ins16", "ins17", "ins_n", "complex", "same_ins0", "across")  # _two_segment_reads' cycle
N_KINDS = 22


def event_world(n_reads, seed):
    """one single-segment read, then n_reads two-segment reads drawn from 22: the ten planted reads of host_lists as the '+' walk saw
    them, the same ten as the '-' walk of an index with add_revcomp saw them (REV records, strand 2), and the two reverse-complemented
    homopolymer reads as the '+' walk saw them (REV records, strand 1: MINUS) - records that name 23 sequences again and again
    -> (host_lists' dict, sequences, offsets, records, the kind of every two-segment read)"""
    h = dict(host_lists(K, True, K, False, 100), k=K)
    fs, _, fr = _two_segment_reads(h, 1, 10, strand=1)
    rs, _, rr = _two_segment_reads(h, 0, 10, strand=2)
    assert not (fr["flags"][1:] & 1).any() and (rr["flags"] & 1).all() and (rr["strand"] == 2).all() and len(fr) == 21 and len(rr) == 20
    rr = rr.copy()
    rr["seq"] += len(fs)
    seqs, more = fs + rs, []
    for name in ("hp_del_rc", "hp_ins_rc"):
        i = h["names"].index(name)
        mine = h["segs"][0][h["segs"][0]["seq"] == i].copy()
        assert len(mine) == 2 and (mine["flags"] & 1).all() and (mine["strand"] == 1).all(), name
        mine["seq"] = len(seqs)
        seqs.append(h["strand_seqs"][0][i])
        more.append(mine)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    pairs = np.concatenate([fr[1:], rr] + more).reshape(N_KINDS, 2)
    which = np.random.default_rng(seed).integers(0, N_KINDS, n_reads)
    which[:2 * N_KINDS] = np.arange(2 * N_KINDS) % N_KINDS
    which[(SCAN_TURN - 1) // 2] = 0  # the insertion read: its pair lies across record 524 288
    recs = np.concatenate([fr[:1], pairs[which].reshape(-1)])
    return h, seqs, off, recs, which


def test_event_scan_over_more_than_one_round_of_the_sums():
    import torch
    sbwt = _located(K, True)
    n_reads = (SCAN_TURN + 2 * CHUNK) // 2 - 100
    h, seqs, off, recs, which = event_world(n_reads, 11)
    cat, soff = np.concatenate(seqs), h["soff"]
    n_recs = len(recs)
    assert n_recs > SCAN_TURN + CHUNK and (n_recs + CHUNK - 1) // CHUNK == SCAN_ROUND + 2, "event_sums_kernel takes a second round over two chunks"
    assert recs["seq"][SCAN_TURN - 1] == recs["seq"][SCAN_TURN], "a junction pair lies across record 524 288"
    want, cx, at = vector_events(recs, cat, off, K, soff, False, 100)
    n = len(want)
    # the statement is the definition's: brute force over the first 3 000 records
    check = []
    made, bcx = brute_events(recs[:3000], seqs, off, K, soff, False, 100, check, 3000)
    few = int((at < 3000).sum())
    assert made == few == len(check) and event_tuples(want[:few]) == check and bcx == int(vector_events(recs[:3000], cat, off, K, soff, False, 100)[1]) > 100
    cx_at = np.flatnonzero(np.isin(which, [READS.index("complex"), 10 + READS.index("complex")])) * 2 + 2  # the record a complex junction's pair ends at
    for chunk in (SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1):
        mine = want[at // CHUNK == chunk]
        assert len(mine) > 300 and (mine["kind_len"] & INS).any() and not (mine["kind_len"] & INS).all() and (mine["kind_len"] & LONG).any(), chunk
        assert (mine["flags"] == 1).any() and (mine["flags"] == 0).any() and (cx_at // CHUNK == chunk).sum() > 40, chunk
    assert SCAN_TURN in at and cx == len(cx_at), "the pair across record 524 288 is an event"
    stream = torch.cuda.Stream()
    # (records taken, *d_n_segs, event capacity, events already in the list)
    runs = ((SCAN_TURN, n_recs, None, 0),      # one round: the control
            (SCAN_TURN + 1, n_recs, 0, 0),     # the smallest capacity with 257 chunks, the last one's only pair an event
            (n_recs, n_recs, 4, 0), (n_recs, n_recs + 1000, 0, 0), (n_recs, n_recs, -n // 2, 0), (n_recs, n_recs, 8, 3))
    for run, (cap, count, spare, before) in enumerate(runs):
        w = want[at < cap]
        host, hn, hcx = locate.indels_from_segments_host(recs[:cap], cat, off, K, soff, skip_multi=False, max_indel=100)
        assert hn == len(w) and host[:hn].tobytes() == w.tobytes() and hcx == int((cx_at < cap).sum())
        if cap == SCAN_TURN + 1:
            assert (cap + CHUNK - 1) // CHUNK == SCAN_ROUND + 1 and len(w) == len(want[at < SCAN_TURN]) + 1, "an event in chunk 257, and one alone"
        ecap = before + len(w) + (4 if spare is None else spare)
        p = _Lists(sbwt, cap, ecap, 0, seed=run, n_events=before)
        head = p.events.host().view(locate.INDEL_EVENT_DTYPE)[:before].copy()
        _Uploaded(sbwt, seqs, off, recs, capacity=cap, count=count, seed=run).run(p, False, 100, stream=stream)  # (checks the inputs)
        ev, ne, _, _ = p.results("run %d" % run)
        assert ne == before + len(w), (run, ne, before + len(w))
        assert ev[:before].tobytes() == head.tobytes() and ev[before:].tobytes() == w[:ecap - before].tobytes(), (run, _differ(ev[before:], w[:ecap - before]))


# ---- 2. the head and site scans over more than one round
INS16 = 16 | INS
SITE_POS = (0, 4500, 8999, 9000)
SITE_DEPTH = {0: 0, 4499: 3, 8998: 200, 8999: 2}  # DEPTH[pos - 1]: at (1, 1, 2) every group, groups of 2 and more, of 100 and more, every group (at equality)
T_SCAN = (1, 1, 2)


def group_world(n_groups, seed):
    """insertions of 16 bases with distinct codes at four positions, listed in key order: -> (events, the size of every group, the place
    its first event takes).  Most groups hold one event; groups of 2, 64 and 65 lie in front of place 524 288 and behind it, one of
    CHUNK + 52 across it.  MINUS: every third event of a group, every third group of one"""
    rng = np.random.default_rng(seed)
    share = (n_groups // 5, n_groups // 5, n_groups // 5, n_groups - 3 * (n_groups // 5))
    pos = np.repeat(SITE_POS, share)
    code = np.concatenate([np.unique(rng.integers(0, 1 << 32, 2 * m, dtype=np.uint64))[:m] for m in share])
    assert len(code) == n_groups
    size = np.ones(n_groups, dtype=np.int64)
    big = SCAN_TURN - 1000 - (1 + 63 + 64 + 1)  # (its first place is 524 288 - 1 000: the groups in front of it hold 129 events more than one each)
    for g, m in ((5, 2), (3000, 64), (250_000, 65), (400_000, 2), (big, CHUNK + 52), (big + 1500, 2), (big + 2000, 64), (big + 2500, 65), (big + 3000, 1), (n_groups - 1, 2)):
        size[g] = m
    first = np.concatenate([[0], np.cumsum(size)])
    g = np.repeat(np.arange(n_groups), size)
    j = np.arange(first[-1]) - first[g]
    ev = np.zeros(first[-1], dtype=locate.INDEL_EVENT_DTYPE)
    ev["pos"], ev["kind_len"], ev["code"] = pos[g], INS16, code[g]
    ev["flags"] = np.where(size[g] == 1, g % 3 == 0, j % 3 == 0)
    return ev, size, first[:-1]


def test_head_and_site_scans_over_more_than_one_round():
    import torch
    sbwt = _located(K, False)
    soff = host_lists(K, False, K, False, 100)["soff"]
    n_bases = int(soff[-1])
    assert n_bases == SITE_POS[-1] == 9000
    n_groups = SCAN_TURN + 2 * CHUNK + 300
    sorted_ev, size, first = group_world(n_groups, 3)
    n = len(sorted_ev)
    last = first + size - 1
    assert n > n_groups > SCAN_TURN + 2 * CHUNK, "sums64_kernel and site_sums_kernel both take a second round over more than two chunks"
    for m in (1, 2, 64, 65):
        assert ((size == m) & (last < SCAN_TURN)).any() and ((size == m) & (first > SCAN_TURN)).any(), m
    big = int(np.argmax(size))
    assert size[big] > CHUNK and first[big] < SCAN_TURN - 900 and last[big] > SCAN_TURN + 900, "a group of more than a chunk straddles place 524 288"
    depth = np.full(n_bases, 77, dtype=np.uint32)
    for at, d in SITE_DEPTH.items():
        depth[at] = d
    ev = sorted_ev[np.random.default_rng(4).permutation(n)]
    stream = torch.cuda.Stream()
    assert n - SCAN_TURN > 3 * CHUNK
    # (event capacity, site capacity: 1 at the count, 2 half of it, 0 none, thresholds)
    runs = ((SCAN_TURN, 1, T_SCAN), (SCAN_TURN + 1, 2, T_SCAN), (n, 1, T_SCAN), (n, 2, T_SCAN), (n, 0, T_SCAN), (n + 3 * CHUNK + 5, 1, T_SCAN), (n, 1, (2, 0, 1)))
    groups = {}
    for run, (ecap, part, t) in enumerate(runs):
        lst = ev[:ecap]
        if len(lst) not in groups:
            groups[len(lst)] = vector_groups(lst, n_bases)
        want, u, cnt = vector_sites(lst, depth, soff, *t, groups=groups[len(lst)])
        host, hn = locate.indel_sites_host(lst, n, depth, soff, min_count=t[0], frac_num=t[1], frac_den=t[2])
        assert hn == len(want) and host.tobytes() == want.tobytes()
        assert events_hold(lst, n_bases).all() and len(u) > SCAN_TURN - 3 * CHUNK
        minus, heads = int(lst["flags"].sum()), len(u)
        assert 0 < minus < heads, "the high word of the packed sum is neither zero nor the head count"
        if ecap == SCAN_TURN:
            assert len(lst) == ecap, "every place holds a key: the end marker is the only place of chunk 257"
        if ecap >= n:
            assert len(u) == n_groups and np.array_equal(cnt, size), "np.unique finds the groups as they were made"
            passes = np.flatnonzero((cnt >= t[0]) & (cnt * t[2] >= t[1] * depth[np.maximum(u[:, 0] - 1, 0)].astype(np.int64)))
            assert len(passes) == len(want) and (passes > SCAN_TURN).sum() > (1000 if t == T_SCAN else 3), "sites beyond group 524 288"
            assert 0 < len(want) < n_groups and (t != T_SCAN or len(want) > SCAN_TURN // 2)
            if run == 2:  # the statement is the definition's: brute force over a sample of the list with whole groups in it
                pick = np.flatnonzero(np.isin(ev["code"], sorted_ev["code"][np.concatenate([first[::400], first[size > 1]])]))
                assert 3000 < len(pick) < 9000
                assert site_tuples(vector_sites(ev[pick], depth, soff, *t)[0]) == brute_sites(event_tuples(ev[pick]), depth, soff, *t)
        scap = (0, len(want), len(want) // 2)[part]  # (none, at the count, half of it)
        sites, ns = _sites_on_device(sbwt, lst, n, depth, ecap, scap, t, stream, seed=run)
        assert ns == len(want) and sites.tobytes() == want[:scap].tobytes(), (run, ns, len(want), _differ(sites, want[:scap]))


# ---- 3. every pass count and both buffer parities
_small = {}


def small_handle(lens):
    """a located handle at k = 5 over random sources of these lengths"""
    if lens not in _small:
        rng = np.random.default_rng(sum(lens))
        srcs = [ACGT[rng.integers(0, 4, n)] for n in lens]
        _small[lens] = (kbo_amd.add_positions(_build(srcs, 5, False, "host"), srcs, add_revcomp=False), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    return _small[lens]


def handle(which):
    """(handle, source offsets, (passes, bits of the top digit) as the test expects them)"""
    if which == "9 passes":
        return small_handle((120, 0, 79)) + ((9, 8),)
    if which == "10 passes, 1 bit":
        return small_handle((150, 1, 160)) + ((10, 1),)
    if which == "10 passes, 6 bits":
        return _located(K, False), host_lists(K, False, K, False, 100)["soff"], (10, 6)
    sbwt, _, soff = big_handle()
    return sbwt, soff, (11, 5)


def pass_events(n_bases, n, seed):
    """a shuffled list of n events drawn by `seed` - the same draws for every handle, the positions scaled to its bases: deletions and
    insertions of every kind at pos 0, pos == n_bases, positions with the top pos bit set and others, groups of up to 9 equal events,
    MINUS in some, and a few words that hold no event"""
    rng = np.random.default_rng(seed)
    m = n // 3
    top = 1 << (pos_bits(n_bases) - 1)
    frac = rng.random(m)
    pos = np.where(frac < 0.5, (frac * 2 * top).astype(np.int64), top + ((frac - 0.5) * 2 * (n_bases - top + 1)).astype(np.int64))
    pos[:6] = (0, 0, n_bases, n_bases, top, n_bases - 1)
    kind = rng.integers(0, 4, m)
    kind[:6] = (0, 1, 1, 2, 0, 0)
    ln = np.where(kind == 0, rng.integers(1, 6, m), np.where(kind == 1, rng.integers(1, 16, m), np.where(kind == 2, 16, rng.integers(17, 3000, m))))
    code = np.where((kind == 1) | (kind == 2), rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.int64) & ((1 << (2 * np.minimum(ln, 16))) - 1), 0)
    kl = ln | np.where(kind > 0, INS, 0) | np.where(kind == 3, LONG, 0)
    g = np.concatenate([np.arange(m), rng.integers(0, m, n - m)])  # every key once, then again at random
    ev = np.zeros(n, dtype=locate.INDEL_EVENT_DTYPE)
    ev["pos"], ev["kind_len"], ev["code"], ev["flags"] = pos[g], kl[g], code[g], rng.integers(0, 2, n)
    ev["flags"][rng.integers(0, n, 20)] = 2       # no event
    ev["kind_len"][rng.integers(0, n, 20)] &= ~np.uint32(LEN_MASK)
    return ev[rng.permutation(n)]


@pytest.mark.parametrize("which", ["9 passes", "10 passes, 1 bit", "10 passes, 6 bits", "11 passes"])
def test_every_pass_count_and_both_buffer_parities(which):
    import torch
    sbwt, soff, expect = handle(which)
    n_bases = int(soff[-1])
    assert np.array_equal(sbwt.source_offsets(), soff) and sort_passes(n_bases) == expect, (n_bases, sort_passes(n_bases))
    if which in ("9 passes", "11 passes"):
        assert sort_passes(n_bases)[0] % 2 == 1, "`sort_passes` is odd: the sorted keys end in the second buffer"
    n = RADIX_SCAN_TURN + TILE + 9
    assert n > RADIX_SCAN_TURN, "more than one block of the scan under a radix pass, a last tile of 9 keys"
    ev = pass_events(n_bases, n, 21)
    held = events_hold(ev, n_bases)
    top = 1 << (pos_bits(n_bases) - 1)
    assert 30 < (~held).sum() < n // 4 and (ev["pos"][held] == 0).any() and (ev["pos"][held] == n_bases).any() and (ev["pos"][held] >= top).sum() > n // 4
    depth = np.random.default_rng(5).integers(0, 12, n_bases).astype(np.uint32)
    stream = torch.cuda.Stream()
    for t in (T_ALL, (2, 1, 2)):
        want, u, cnt = vector_sites(ev, depth, soff, *t)
        host, hn = locate.indel_sites_host(ev, n, depth, soff, min_count=t[0], frac_num=t[1], frac_den=t[2])
        assert hn == len(want) and host.tobytes() == want.tobytes() and site_tuples(want) == brute_sites(event_tuples(ev), depth, soff, *t)
        assert 100 < len(want) and (t == T_ALL or len(want) < len(u)) and cnt.max() >= 4 and (want["pos"] == 0).any() and (want["pos"] == n_bases).any()
        for ecap, scap in ((n, len(want)), (n + 77, len(want) // 2)):
            sites, ns = _sites_on_device(sbwt, ev, n, depth, ecap, scap, t, stream, seed=ecap % 89)
            assert ns == len(want) and sites.tobytes() == want[:scap].tobytes(), (which, t, ecap, _differ(sites, want[:scap]))


# ---- 4. a ladder over every sorted key bit
def ladder(n_bases):
    """for every bit the sort goes over a pair of events that event_key() accepts and whose keys differ in that bit alone - but for
    kind_len's bit 30 (LONG), which only moves together with the length: 16 bases and code 0 against 17 bases, LONG, differ in bits 30,
    4 and 0 of kind_len.  A rung of kind_len or code sits at a position of its own, a rung of pos carries a code of its own: no two rungs
    share a key -> [(name, low key, high key)], a key (pos, kind_len, code)"""
    rungs = []
    for b in range(pos_bits(n_bases)):
        rungs.append(("pos bit %d" % b, (0, INS16, b + 1), (1 << b, INS16, b + 1)))
    for b in range(30):  # LONG insertions with code 0: both lengths above 16
        base = 64 if b < 6 else 32
        rungs.append(("kind_len bit %d" % b, (100 + b, INS | LONG | base, 0), (100 + b, INS | LONG | base | 1 << b, 0)))
    rungs.append(("kind_len bit 30, with bits 4 and 0", (130, INS | 16, 0), (130, INS | LONG | 17, 0)))
    rungs.append(("kind_len bit 31", (131, 1, 0), (131, INS | 1, 0)))  # a deletion and an insertion of one base, code 0
    for b in range(32):
        rungs.append(("code bit %d" % b, (200 + b, INS16, 0), (200 + b, INS16, 1 << b)))
    return rungs


@pytest.mark.parametrize("which", ["10 passes, 6 bits", "11 passes"])
def test_a_ladder_over_every_sorted_key_bit(which):
    import torch
    sbwt, soff, expect = handle(which)
    n_bases = int(soff[-1])
    assert sort_passes(n_bases) == expect
    rungs = ladder(n_bases)
    assert len(rungs) == pos_bits(n_bases) + 32 + 32, "every bit launch_indel_sites sorts: the pos bits of the handle, kind_len, code"
    for name, lo, hi in rungs:
        w = [(a ^ b) for a, b in zip(lo, hi)]
        field = ("pos", "kind_len", "code").index(name.split()[0])
        assert sum(1 for x in w if x) == 1 and (bin(w[field]).count("1") == 1 or "with bits" in name) and w[field] >> int(name.split()[2].rstrip(",")) & 1, name
        assert lo < hi and hi[0] <= n_bases
    keys = sorted({key for _, lo, hi in rungs for key in (lo, hi)})
    assert len(keys) == 2 * len(rungs), "no two rungs share a key"
    # descending key order, a key once or three times, MINUS in the first of the three
    count = {key: 3 if i % 2 else 1 for i, key in enumerate(keys)}
    rows = [key + (1 if c == 3 and j == 0 else 0,) for key in reversed(keys) for c in (count[key],) for j in range(c)]
    ev = _events(rows)
    assert events_hold(ev, n_bases).all(), "event_key accepts every rung"
    depth = np.zeros(n_bases, dtype=np.uint32)
    want, _, _ = vector_sites(ev, depth, soff, *T_ALL)
    assert [(int(s["pos"]), int(s["kind_len"]), int(s["code"]), int(s["count"]), int(s["n_minus"])) for s in want] == [
        key + (count[key], 1 if count[key] == 3 else 0) for key in keys], "ascending (pos, kind_len, code), the counts as listed"
    host, hn = locate.indel_sites_host(ev, len(ev), depth, soff, min_count=1, frac_num=0, frac_den=1)
    assert hn == len(keys) and host.tobytes() == want.tobytes() and site_tuples(want) == brute_sites(event_tuples(ev), depth, soff, *T_ALL)
    stream = torch.cuda.Stream()
    for ecap in (len(ev), len(ev) + 5):
        sites, ns = _sites_on_device(sbwt, ev, len(ev), depth, ecap, len(keys), T_ALL, stream, seed=ecap)
        if sites.tobytes() != want.tobytes():
            got = [(int(s["pos"]), int(s["kind_len"]), int(s["code"])) for s in sites]
            wrong = [name for name, lo, hi in rungs if lo not in got or hi not in got or got.index(lo) > got.index(hi)]
            raise AssertionError("%s, event capacity %d: %d sites for %d; rungs out of order: %s" % (which, ecap, ns, len(keys), wrong[:12]))
        assert ns == len(keys)


# ---- 5. thresholds and ends on the device
def test_thresholds_in_64_bits_and_events_at_both_ends():
    import torch
    lens = (0, 40, 0, 0, 60, 0)
    sbwt, soff = small_handle(lens)
    n_bases = int(soff[-1])
    assert n_bases == 100 and (np.diff(soff.astype(np.int64)) == 0).sum() == 4, "sources of length 0 at base 0, at base 40 (two) and at the end"
    M = 0xFFFFFFFF
    depth = np.zeros(n_bases, dtype=np.uint32)
    depth[0], depth[9], depth[19], depth[39], depth[59], depth[99] = M, 3, M, 0x80000001, 6, 2
    rows = [(0, 1, 0, 1)] * 3 + [(0, 1 | INS, 2, 0)] * 2        # pos 0 reads DEPTH[0]
    rows += [(1, 2, 0, 0)] * 3 + [(1, 1 | INS, 1, 0)] * 2       # pos 1 reads it too
    rows += [(10, 1, 0, 0)] * 3 + [(10, 2, 0, 1)] * 2           # DEPTH[9] = 3
    rows += [(20, 1 | INS, 3, 0)] * 4 + [(20, 3, 0, 0)]         # DEPTH[19] = 2^32 - 1
    rows += [(40, 1 | INS, 0, 0)] * 3 + [(40, 2, 0, 0)] * 2     # the first base of source 4, behind two empty sources: DEPTH[39] = 2^31 + 1
    rows += [(60, 5, 0, 0)] * 3                                 # DEPTH[59] = 6
    rows += [(100, 1 | INS, 1, 1)] * 3 + [(100, 17 | INS | LONG, 0, 0)] * 2 + [(100, 1, 0, 0)] * 3  # pos == source_bases: a deletion there holds no event
    ev = _events(rows)[np.random.default_rng(2).permutation(len(rows))]
    stream = torch.cuda.Stream()
    seen = set()
    # (min_count, frac_num, frac_den): count * frac_den against frac_num * depth, each beyond 32 bits somewhere, at equality and one below
    for t in ((1, 3, M), (1, M, M), (2, 0x80000000, 1), (1, 1, 0x80000000), (1, 2, M), (3, 1, 2), (1, M, 1)):
        want = brute_sites(event_tuples(ev), depth, soff, *t)  # (Python integers)
        vec, u, cnt = vector_sites(ev, depth, soff, *t)
        host, hn = locate.indel_sites_host(ev, len(ev), depth, soff, min_count=t[0], frac_num=t[1], frac_den=t[2])
        assert site_tuples(vec) == want and hn == len(want) and host.tobytes() == vec.tobytes()
        for key, c in zip(u.tolist(), cnt.tolist()):
            d = int(depth[max(key[0] - 1, 0)])
            left, right = c * t[2], t[1] * d
            if c >= t[0] and (left >> 32 or right >> 32):
                seen.add(("equal" if left == right else "one below" if c * t[2] < right <= (c + 1) * t[2] else "left" if left >> 32 and not right >> 32 else
                          "right" if right >> 32 and not left >> 32 else "both"))
                if (left & M) >= (right & M) and left < right:
                    seen.add("32 bits would call it")
                if (left & M) < (right & M) and left >= right:
                    seen.add("32 bits would miss it")
        sites, ns = _sites_on_device(sbwt, ev, len(ev), depth, len(ev), len(want), t, stream, seed=t[1] % 97)
        assert ns == len(want) and sites.tobytes() == host.tobytes() and site_tuples(sites) == want, (t, site_tuples(sites), want)
        if t == (1, 1, 0x80000000):
            by_pos = {s[0]: s[1] for s in want}
            assert by_pos[0] == 1 and by_pos[40] == 4 and by_pos[100] == 5 and 60 in by_pos, "seq_of passes over the empty sources in front of an event"
            assert not any(s[0] == 100 and not s[2] & INS for s in want), "a deletion at pos == source_bases leaves the sources"
    assert seen >= {"equal", "one below", "left", "right", "both", "32 bits would call it", "32 bits would miss it"}, seen
