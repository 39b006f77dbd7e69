"""Shared pieces of the -m gpu tests (imported by test modules; holds no test itself)."""
import os

import numpy as np

import kbo_amd


def threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def adopt(oracle, sbwt, parts=False):
    """The oracle over the product-built index (its own row-sorting builder needs minutes beyond ~20 Mbp; builder
    equality is tests/test_builder_vs_oracle.py up to 300 kbp, check_rows_off_the_text at any size)."""
    rows, Carr, lcs = sbwt.export_parts()
    ora = oracle.Index.from_parts(sbwt.k(), sbwt.n_sets(), sbwt.n_kmers(), rows, Carr, lcs)
    return (ora, lcs) if parts else ora


def check_rows_off_the_text(oracle, ora, lcs, sbwt, g, n_samples=10_000, seed=7):
    """A check of the index that passes through NEITHER builder (the oracle adopts the product-built index beyond 20 Mbp):
    `g` is one ACGT contig whose k-mers are all distinct (n_sets == len(g) + 1 says so: G - k + 1 k-mers + k dummy rows).
    For a sample of k-mers taken off the text, oracle/index_check.c counts - by a pass over the text alone - how many of
    the text's k-mers are colex-smaller; with the dummy rows `$..$ g[0:j]` that are smaller (direct string comparison) that
    IS the k-mer's row in the index index.rs:56-99 defines.  Checked against it: (1) the interval the product's walk of
    the k-mer ends in (depth k, that single row); (2) the k-mer the subset matrix spells at that row and at its two
    neighbours (oracle access_kmer over the adopted parts: k backward steps over the matrix, no row table): the row's own
    k-mer is the sampled one, the neighbours' ranks counted off the text are row - 1 and row + 1 and they occur in the
    text exactly once; (3) the LCS values of those rows against the common suffixes of the spelled k-mers."""
    from kbo_amd import batch
    k, n, G = sbwt.k(), sbwt.n_sets(), len(g)
    assert n == G + 1
    rng = np.random.default_rng(seed)
    pos = np.unique(np.concatenate([[0, 1, G - k], rng.integers(0, G - k + 1, n_samples)]))
    kmers = np.stack([g[p:p + k] for p in pos])
    less, eq = oracle.kmer_colex_ranks(g, k, kmers, n_threads=threads())
    assert (eq == 1).all()
    head = g[:k].tobytes()
    rev_heads = [head[:j][::-1] for j in range(k)]  # dummy row j = $^(k-j) g[0:j]: smaller iff rev(g[0:j]) <= the k-mer's last j characters reversed

    def dummies_below(km):
        r = km[::-1]
        return sum(1 for j in range(k) if rev_heads[j] <= r[:j])
    rows = np.array([int(l) + dummies_below(km.tobytes()) for l, km in zip(less, kmers)], dtype=np.int64)
    # (1) the product's walk with intervals over the sampled k-mers, one sequence each
    off = np.arange(len(kmers) + 1, dtype=np.uint64) * np.uint64(k)
    d, lo, hi = batch.ms_batch(sbwt, kmers.ravel(), off, want_intervals=True)
    last = (off[1:] - np.uint64(1)).astype(np.int64)
    assert (d[last] == k).all()
    assert np.array_equal(lo[last].astype(np.int64), rows) and np.array_equal(hi[last].astype(np.int64), rows + 1)
    # (2), (3) on a part of the sample (k select steps per spelled row)
    sub = rng.choice(len(rows), size=min(len(rows), 1500), replace=False)
    spelled, want_rank = [], []
    for i in sub:
        r = int(rows[i])
        assert ora.access_kmer(r) == kmers[i].tobytes()
        for rr in (r - 1, r + 1):
            if 0 <= rr < n:
                s = ora.access_kmer(rr)
                if b"$" not in s:
                    spelled.append(np.frombuffer(s, dtype=np.uint8))
                    want_rank.append(rr)
        for rr in (r, r + 1):  # LCS[rr] = longest common suffix of rows rr - 1 and rr ($ matches nothing)
            if 1 <= rr < n:
                a, b = ora.access_kmer(rr - 1), ora.access_kmer(rr)
                c = 0
                while c < k and a[k - 1 - c] == b[k - 1 - c] and a[k - 1 - c] != ord("$"):
                    c += 1
                assert int(lcs[rr]) == c, (rr, a, b)
    if spelled:
        sp = np.stack(spelled)
        l2, e2 = oracle.kmer_colex_ranks(g, k, sp, n_threads=threads())
        assert (e2 == 1).all()
        assert [int(l) + dummies_below(km.tobytes()) for l, km in zip(l2, sp)] == want_rank


def call_walk_sites(L, sbwt, dev, thr):
    """kbo_call_walk_dev over a DeviceBatch -> (set of (offset of i, offset of j, row), MS bytes, usable)"""
    import torch
    lists = 256  # KBO_CALL_LISTS
    cap = (dev.total // 4 + 8192) // lists * lists
    sites = torch.zeros((cap, 4), dtype=torch.int32, device=dev.device)
    count = torch.zeros(lists * 16 + 16, dtype=torch.int32, device=dev.device)
    s = torch.cuda.current_stream(dev.device)
    dev.ms.fill_(0xEE)
    kbo_amd.check(L.kbo_call_walk_dev(sbwt._h, dev.q.data_ptr(), dev.off.data_ptr(), dev.n_seqs, dev.total, dev.max_len, thr,
                                      dev.ms.data_ptr(), sites.data_ptr(), cap, count.data_ptr(), dev.work.data_ptr(),
                                      dev.work_bytes, s.cuda_stream))
    torch.cuda.synchronize()
    c = count.cpu().numpy()
    seg = cap // lists
    ok = bool((c[:lists * 16:16] <= seg).all()) and int(c[lists * 16]) == 0
    h = sites.cpu().numpy().view(np.uint32)
    raw = np.concatenate([h[g * seg:g * seg + min(int(c[g * 16]), seg)] for g in range(lists)])
    raw = raw[raw[:, 0] != 0xFFFFFFFF]
    return {(int(a), int(b), int(r)) for a, b, r, _ in raw}, dev.ms[:dev.total].cpu().numpy(), ok


def oracle_sites(ora, concat, offsets, thr):
    """variant_calling.rs:266-273 for every read (oracle, literal) as the set call_walk_sites returns"""
    recs = ora.call_sites_batch(concat, offsets, thr, n_threads=threads())
    off = np.asarray(offsets, dtype=np.uint64)
    base = off[recs[:, 0].astype(np.int64)]
    return {(int(b + i), int(b + j), int(r)) for b, i, j, r in zip(base, recs[:, 1], recs[:, 2], recs[:, 3])}


RUN_CODE = np.zeros(256, dtype=np.uint8)
RUN_CODE[ord("-")], RUN_CODE[ord("X")], RUN_CODE[ord("R")] = 1, 2, 3


def expected_runs(chars, offsets, min_len=0):
    """maximal runs of one character other than 'M' inside each sequence (numpy), as batch.SPARSE_DTYPE; sequences shorter than
    min_len get none"""
    from kbo_amd import batch
    chars = np.asarray(chars, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    n = len(chars)
    first, last = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    lens = np.diff(off)
    first[off[:-1][lens > 0]] = True
    last[off[1:][lens > 0] - 1] = True
    other = chars != ord("M")
    prev_diff = np.ones(n, dtype=bool)
    prev_diff[1:] = chars[1:] != chars[:-1]
    next_diff = np.ones(n, dtype=bool)
    next_diff[:-1] = chars[:-1] != chars[1:]
    starts = np.nonzero(other & (first | prev_diff))[0]
    ends = np.nonzero(other & (last | next_diff))[0]
    assert len(starts) == len(ends)
    seq = np.searchsorted(off, starts, side="right") - 1
    keep = lens[seq] >= min_len
    out = np.zeros(int(keep.sum()), dtype=batch.SPARSE_DTYPE)
    out["seq"] = seq[keep]
    out["start"] = (starts - off[seq])[keep]
    out["len"] = (ends - starts + 1)[keep]
    out["code"] = RUN_CODE[chars[starts]][keep]
    return out


def long_reads(rng, g, n_reads, read_len, sub_rate):
    """reads of read_len bases off g with substitutions (numpy; synth.reads is for 150 bp reads at scale)"""
    starts = rng.integers(0, len(g) - read_len, n_reads)
    out = np.empty(n_reads * read_len, dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for r, a in enumerate(starts):
        p = g[a:a + read_len].copy()
        hit = rng.random(read_len) < sub_rate
        p[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        out[r * read_len:(r + 1) * read_len] = p
    return out, np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)


def round16(n):
    return (int(n) + 15) // 16 * 16


def scratch_guard_bytes(n_seqs, total, k):
    """back guard of a d_work / scratch buffer: everything the largest figure of any route could reach beyond a buffer declared at the
    smallest one (kbo_work_bytes at max_seq_len = 0 holds every region, plus two shards' MS values)"""
    return int(kbo_amd.lib().kbo_work_bytes(n_seqs, total, 0, k)) + 2 * (round16(total) + 16)


PER_BASE_GUARD = 64 << 10  # back guard of a per-base buffer


class Guarded:
    """A device buffer of exactly `n` bytes inside one torch uint8 tensor laid out [front guard][n bytes][back guard].  The front
    guard is a multiple of 256 bytes, so the buffer keeps torch's alignment.  fill() writes a seeded pseudo-random pattern (never
    zeros) over all of it, then the caller's bytes: `data` at the start of the buffer, `front_bytes` / `back_bytes` as the last bytes of the front guard / the first
    bytes behind `data` (input buffers: bytes that continue the genome, so that a kernel that reads past them changes its results).  check()
    names the first guard byte that changed."""

    def __init__(self, name, n, back, device, front=4096, seed=0, data=None, front_bytes=None, back_bytes=None):
        import torch
        assert front % 256 == 0 and n >= 0 and back >= 0
        self.name, self.n, self.front, self.back = name, int(n), int(front), int(back)
        self.device = device
        self.t = torch.empty(self.front + self.n + self.back, dtype=torch.uint8, device=device)
        self.data, self.front_bytes, self.back_bytes = data, front_bytes, back_bytes
        self.fill(seed)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.front

    @property
    def buf(self):
        return self.t[self.front:self.front + self.n]

    def host(self):
        return self.buf.cpu().numpy()

    def fill(self, seed):
        """every byte from the pattern of `seed`, then the caller's bytes over it; the guards are remembered for check()"""
        import torch
        rng = np.random.default_rng(0x6B626F ^ (seed * 7919) ^ (self.n << 3))
        img = rng.integers(1, 256, len(self.t), dtype=np.uint8)  # (1 .. 255: never a zero byte)
        if self.front_bytes is not None:
            fb = np.asarray(self.front_bytes, dtype=np.uint8)[-self.front:]
            img[self.front - len(fb):self.front] = fb
        if self.data is not None:
            d = np.asarray(self.data, dtype=np.uint8).ravel()
            assert len(d) <= self.n
            img[self.front:self.front + len(d)] = d
        if self.back_bytes is not None:
            bb = np.asarray(self.back_bytes, dtype=np.uint8)
            a = self.front + (len(self.data) if self.data is not None else 0)  # (the buffer's unspecified tail continues as well)
            bb = bb[:len(img) - a]
            img[a:a + len(bb)] = bb
        self.t.copy_(torch.from_numpy(img).to(self.device))
        self.image = self.t.clone()

    def check(self):
        """None, or (side, first changed offset from the guard's start, number of changed bytes)"""
        diff = self.t != self.image
        for side, a, b in (("front", 0, self.front), ("back", self.front + self.n, len(self.t))):
            bad = diff[a:b].nonzero()
            if len(bad):
                return side, int(bad[0]), int(len(bad))
        return None

    def changed(self):
        """any byte of buffer or guards different from what fill() wrote"""
        return bool((self.t != self.image).any())

    def assert_intact(self, what=""):
        r = self.check()
        assert r is None, "%s%s: %s guard changed, first bad byte at guard offset %d, %d bytes changed" % (
            what + ": " if what else "", self.name, r[0], r[1], r[2])


# ---------------------------------------------------------------------------------------------------------------- derandomize + translate
# over MS bytes made by numpy - no index, no walk: arbitrary bytes <= k (tests/test_gpu_derand_seq.py, tests/test_gpu_derand_arbitrary.py)

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
DERAND_CONTENTS = ["uniform", "below", "all_k", "anchors", "walk", "k_last", "k_first"]
DT_PIECE, DT_REACH = 132, 1023  # kDtPiece, kDtLookahead - 1 (derand_kernels.hip): a piece looks at the positions [c1, c1 + DT_REACH]
# sparse_k: distance from the end of the piece behind one k to the next k - just inside and just outside [c1, c1 + 1023], both sides
SPARSE_NEAR = [1023, 1024, 1022, 1025, 1000, 1028, 1016, 1024, 1023, 1012]
SPARSE_INSIDE = [1023, 1022, 1000, 1016, 1023, 1012]


def derand_content(kind, rng, n, k, t, period=128):
    """n MS bytes (values 0 .. k) of one sequence with threshold t; `period`: the granule k_last / k_first put their k at the last /
    first position of (a chunk, a piece, a 16-byte block)"""
    if kind == "uniform":
        return rng.integers(0, k + 1, n, dtype=np.int64).astype(np.uint8)
    if kind == "below":  # nothing fires but the last position: the values count down to -len
        return rng.integers(0, t + 1, n, dtype=np.int64).astype(np.uint8)
    if kind == "all_k":
        return np.full(n, k, dtype=np.uint8)
    if kind == "anchors":  # only values in (t, k): rising and falling ramps.  (t >= k - 1 has no such value: t itself, nothing fires)
        lo, hi = t + 1, k - 1
        if lo > hi:
            return np.full(n, t, dtype=np.uint8)
        span = hi - lo
        p = np.arange(n) + int(rng.integers(0, 1000))
        tri = np.abs((p % (2 * span + 2)) - (span + 1)).clip(0, span) if span else np.zeros(n, dtype=np.int64)
        return (lo + tri).astype(np.uint8)
    if kind == "walk":  # k, with ramps 0, 1, 2, ... behind mismatches every about 100 bases
        a = np.full(n, k, dtype=np.int64)
        p = int(rng.integers(0, 100))
        while p < n:
            m = min(k, n - p)
            a[p:p + m] = np.arange(m)
            p += int(rng.integers(k // 2 + 1, 200))
        return a.astype(np.uint8)
    base = rng.integers(0, k, n, dtype=np.int64)  # 0 .. k - 1
    if kind == "sparse_k":
        # single k's 1000 .. 1160 positions apart: behind a k at p the next one lies d positions above the end c1 of the piece that
        # holds p (pieces of DT_PIECE positions from the sequence's start), d cycling through values around DT_REACH - so the gap
        # d + (c1 - p) sweeps 1000 + 1 .. 1028 + 132 as p's place inside its piece moves.  Every other sequence draws only d <=
        # DT_REACH: none of its pieces gives up.
        cyc = SPARSE_NEAR if rng.integers(0, 2) else SPARSE_INSIDE
        i, p = int(rng.integers(0, len(cyc))), int(rng.integers(0, 200))
        while p < n:
            base[p] = k
            p = (p // DT_PIECE + 1) * DT_PIECE + cyc[i % len(cyc)]
            i += 1
        return base.astype(np.uint8)
    pos = np.arange(n)
    base[pos % period == (period - 1 if kind == "k_last" else 0)] = k  # the last / first position of every granule
    return base.astype(np.uint8)


def piece_gives_up(ms, k, reach=DT_REACH, piece=DT_PIECE):
    """the piece rule of derand_translate_piece_lds_kernel for one sequence: the ends c1 < len of its pieces, the distance from each
    to the nearest k at or above it (the last position where there is none), and whether the piece gives up - neither a k nor the
    last position in [c1, c1 + reach].  A sequence with one such piece is redone by one lane."""
    n = len(ms)
    c1 = np.arange(piece, n, piece)
    nxt = np.where(np.asarray(ms) == k, np.arange(n), n - 1)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]  # nearest k at or above p, else the last position
    d = nxt[c1] - c1
    return c1, d, d > reach


def compare_chars(got, exp, keep, off, what):
    bad = np.flatnonzero((got != exp) & keep)
    if len(bad):
        p = int(bad[0])
        s = int(np.searchsorted(off, p, side="right") - 1)
        raise AssertionError("%s: %d characters differ, first at sequence %d (%d bases) position %d: got %r, expected %r" % (
            what, len(bad), s, int(off[s + 1] - off[s]), p - int(off[s]), chr(got[p]), chr(exp[p])))


def oracle_chars(ora, ms, off, k, t, ref):
    """oracle.translate_ms_vec(oracle.derandomize_ms_vec(ms_s, k, t), k, t) of every sequence of 3 bases or more, relative_to_ref of it,
    and which bytes these are (the others - sequences of 0, 1 and 2 bases - are unspecified)"""
    total = int(off[-1])
    plain, rel, keep = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=bool)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        if b - a < 3:
            continue
        ch = ora.translate_ms_vec(ora.derandomize_ms_vec(ms[a:b], k, t), k, t).encode()
        plain[a:b] = np.frombuffer(ch, dtype=np.uint8)
        rel[a:b] = np.frombuffer(ora.relative_to_ref(ref[a:b].tobytes(), ch), dtype=np.uint8)
        keep[a:b] = True
    return plain, rel, keep


def derand_thresholds(k):
    """{2, 3, ceil(k / 2), k - 1, k} clipped to 2 .. k"""
    return sorted({min(max(t, 2), k) for t in (2, 3, (k + 1) // 2, k - 1, k)})


DT_TINY = [1, 2, 0, 2, 1]  # sequences of 0, 1 and 2 bases: 6 bytes, so that what follows them starts inside the batch's first 16 bytes
DT_READS = [150, 37, 480, 100]


def piece_lengths(order, seed):
    """the batch of the piece route: every length at which a piece, a wave of 64 pieces or the look-ahead begins or ends, reads and
    sequences of 0, 1 and 2 bases between them.  order 0: tiny sequences first (the first wave's span begins inside the batch's first
    16 bytes, nothing staged below it, and the first real sequence starts at byte 6); 1: the longest first; 2: the longest last (its
    pieces' look-ahead is capped by total_bases)"""
    P = DT_PIECE
    mid = [P - 1, P, P + 1, 2 * P, 2 * P + 1, 481, 64 * P - 1, 64 * P, 64 * P + 1, 1024 + P - 1, 1024 + P, 1024 + P + 1, 20_000]
    rng = np.random.default_rng(seed)
    body = []
    for i, n in enumerate(mid[j] for j in rng.permutation(len(mid))):
        body += [n, DT_TINY[i % 5], DT_READS[i % 4]]
    if order == 0:
        return DT_TINY + body + [70_000, 5]
    if order == 1:
        return [70_000] + body + DT_TINY
    return [3] + body + DT_TINY + [70_000]


LDS_MAX_LENS = [3, 31, 32, 150, 256, 479, 480]
LDS_SEQS = 391  # 7 waves: a last wave of 7 sequences, and a last workgroup that is not full at 2, 3 and 4 waves a workgroup
LDS_FULL_WAVE = (128, 192)  # these 64 sequences all have the maximal length: the largest span the LDS image is sized for


def lds_lengths(mx, variant, seed):
    """the batch of the LDS route for reads of at most mx bases: lengths from {0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, ..., mx - 1,
    mx}, one whole wave at mx; variant 0: the first sequence 1 base, the last one mx, total_bases mod 16 = 0; variant 1: the first
    one mx, the last one 2 bases, total_bases mod 16 = 7"""
    rng = np.random.default_rng(seed)
    cand = sorted({c for c in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, mx - 1, mx) if c <= mx})
    lens = rng.choice(cand, LDS_SEQS)
    lens[LDS_FULL_WAVE[0]:LDS_FULL_WAVE[1]] = mx
    lens[0], lens[-1] = (1, mx) if variant == 0 else (mx, 2)
    target = 0 if variant == 0 else 7
    for i in range(LDS_SEQS - 2, LDS_FULL_WAVE[1], -1):  # a base less for one sequence after the other until the total fits
        if (int(lens.sum()) - target) % 16 == 0:
            break
        if lens[i] > 0:
            lens[i] -= 1
    assert int(lens.sum()) % 16 == target and int(lens.max()) == mx
    return [int(n) for n in lens]


def lds_waves_per_workgroup(mx):
    """launch_derand_translate's choice (derand_kernels.hip): as many waves, at most 4, as 64 KiB of LDS hold"""
    lds = (64 * mx + 15) // 16 * 16 + 16
    wave = ((lds + lds // 32 + 16 if mx % 32 == 0 else lds) + 15) // 16 * 16
    return max(1, min(4, 65536 // wave))


def derand_world(ora, lens, k, t, kind, period, seed):
    """(offsets, MS bytes, reference bytes, the oracle's characters, those relative to the reference, which bytes are specified)"""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    ms = np.concatenate([derand_content(kind, rng, n, k, t, period) for n in lens] + [np.zeros(0, dtype=np.uint8)])
    ref = ACGT[rng.integers(0, 4, int(off[-1]))]
    plain, rel, keep = oracle_chars(ora, ms, off, k, t, ref) if ora is not None else (None, None, None)
    for v in (off, ms, ref, plain, rel, keep):
        if v is not None:
            v.setflags(write=False)
    return off, ms, ref, plain, rel, keep
