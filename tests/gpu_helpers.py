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
