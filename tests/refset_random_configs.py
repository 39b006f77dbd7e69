"""The generator of the second randomized oracle soak, over the reference-set entry points (imported by
tests/test_refset_random_configs_host.py, tests/test_gpu_refset_random_configs.py and tools/stress.py; holds no test itself).
config(seed) draws everything one iteration checks - k by class, the set's add_revcomp, the references by kind and in a drawn order,
max_wide_rows, prefilter and positions, the batch's shape, max_error_prob, max_gap_len, strands, every knob and capacity, which
optional legs run - and make_inputs(cfg) makes the bytes.  Pure numpy: no GPU, no product library, no oracle; the same seed gives the
same bytes on any machine.

What the draws are for (kbo_amd/csrc/refset_plan.hpp, refset_call_kernels.hip, refset_resolve_kernels.hip, refset_screen.hpp): the
chunk max(256, 4k) is no multiple of 16 for most k > 64; the call's match and resolve kernels take one round of 64 lanes more at k =
64 / 65, 128 / 129 and 192 / 193; a window record is k rounded up to 16; below k = 11 no reference can be screened and below 24 the
seed length can be k itself.  K_CLASSES (tests/random_configs.py) gives every one of these its share."""
from dataclasses import dataclass

import numpy as np

from random_configs import ACGT, K_CLASSES, k_class  # noqa: F401 (k_class: for the modules that count the classes)

COMP = np.arange(256, dtype=np.uint8)  # kbo_hip.h kbo_revcomp_batch: a <-> t, c <-> g too (lower case is no base on either strand)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b
CHUNK, MAX_ROWS, WIDE_MAX_ROWS = 256, 16384, 1 << 20  # KBO_REFSET_CHUNK, KBO_REFSET_MAX_ROWS, KBO_REFSET_WIDE_MAX_ROWS
SEED_MAX, SEED_MIN = 24, 11                          # KBO_REFSET_SEED_MAX, KBO_REFSET_SEED_MIN
TASK_ITEMS = 256                                     # refset_plan.hpp kTaskItems: chunks of one task of the walk
LONG_MIN_K = 16  # long references, the contig of more than 256 chunks and the one above 65 536 bases are drawn for k >= 16 only: below,
#                  every k-mer of a long random text is in every reference and the records of a pair grow with its length
KINDS = ("short", "k", "k1", "2k", "n_lower", "twin", "two_letter")  # + "spread" as often as the count asks for, + "long"
KIND_P = {"short": 0.5, "k": 0.45, "k1": 0.45, "2k": 0.5, "n_lower": 0.5, "twin": 0.45, "two_letter": 0.4}
# d: the screen alone; e: locate; f: cover; g: call; h: the device forms of find / summary / best; i: the device forms of call
LEGS = ("d", "e", "f", "g", "h", "i")
LEG_P = {"d": 0.6, "e": 0.5, "f": 0.5, "g": 0.7, "h": 0.6, "i": 0.7}
OPS = ("exact", "sub1", "sub3", "ins2", "del3", "rc")


def chunk_of(k):
    """refset_plan.hpp chunk_of: the bases between two cuts of a sequence"""
    return max(CHUNK, 4 * k)


def revcomp(a):
    return COMP[a[::-1]]


@dataclass
class Config:
    seed: int
    k: int
    add_revcomp: bool          # of the set
    kinds: tuple               # one name per reference, in the set's order ("twin" twice: the two identical ones)
    ref_lens: tuple
    wide_rows: int             # max_wide_rows of the build
    long_route: str            # "none": no long reference; "wide": all of them within wide_rows; "index": the largest one above it
    prefilter: bool
    positions: bool
    n_seqs: int                # sequences of the host batch (all of 3 bases or more)
    many_chunks: bool          # a contig of more than 256 chunks
    huge: bool                 # a contig of more than 65 536 bases
    sources: tuple             # the reference each planted copy is taken from, see _plan()
    order: tuple               # the drawn order of the batch's sequences
    short_seqs: tuple          # (where, length 0 / 1 / 2): put into the batch of the device legs only
    max_error_prob: float      # 1e-7 or 1e-4: every leg
    find_prob: float           # max_error_prob, or 0.5: legs a, b, c, d and h
    max_gap_len: int
    strands: int
    slab_bytes: int            # kbo_set_slab_bytes
    record_capacity: int       # kbo_set_refset_record_capacity
    refs_per_slab: int         # 0: all
    caps: str                  # the screened forms' caps: "ample", "pairs" (max_pairs below the candidates), "bases" (max_pair_bases tight)
    capacity: str              # the device forms' outputs: "ample", "exact", "below"
    max_sites: str             # "ample", "below"
    call_add_revcomp: bool     # add_revcomp of the call's own options.  It puts the reverse complement of the sequence into the sequence's own
                               # index, so it changes a record only where a stretch of a site's k-mer of at least the threshold's length occurs
                               # reverse-complemented in the same contig.  Drawn only where that is not planted and unlikely by chance: k >= 32,
                               # the reverse-complemented copy's reference has no other copy in its contig, no reference over two letters (a
                               # text over A and T meets its own reverse complement often) and max_error_prob 1e-7 (thresholds of 11 and
                               # more; at 1e-4 a reference of k bases has 6).  The host module asserts the outcome for every such seed of SEEDS
    legs: dict

    @property
    def device_leg(self):
        return any(self.legs[n] for n in ("h", "i")) or (self.legs["d"] and self.prefilter) or \
            (self.positions and (self.legs["e"] or self.legs["f"]))

    @property
    def more_than_256_chunks(self):
        """some sequence is cut into more than 256 chunks: a second task per reference"""
        return self.many_chunks or (self.huge and TASK_ITEMS * chunk_of(self.k) < 65536 + 3000)

    @property
    def above_65536(self):
        """some sequence has more than 65 536 bases (the contig of more than 256 chunks has: 258 chunks of 256 bases or more)"""
        return self.huge or self.many_chunks

    def describe(self):
        return ("seed=%d k=%d rc=%s refs=%d kinds=%s wide_rows=%d long=%s prefilter=%s positions=%s n_seqs=%d many_chunks=%s huge=%s "
                "shorts=%s p=%g find_p=%g gap=%d strands=%d slab=%d reccap=%d rps=%d caps=%s capacity=%s max_sites=%s call_rc=%s legs=%s"
                % (self.seed, self.k, self.add_revcomp, len(self.kinds), ",".join(self.kinds), self.wide_rows, self.long_route, self.prefilter,
                   self.positions, self.n_seqs, self.many_chunks, self.huge, self.short_seqs, self.max_error_prob, self.find_prob,
                   self.max_gap_len, self.strands, self.slab_bytes, self.record_capacity, self.refs_per_slab, self.caps, self.capacity,
                   self.max_sites, self.call_add_revcomp, [n for n in LEGS if self.legs[n]]))


def _ref_len(rng, kind, k):
    if kind == "short":
        return k - 1
    if kind == "k":
        return k
    if kind == "k1":
        return k + 1
    if kind == "2k":
        return 2 * k
    if kind == "long":
        return int(rng.integers(17_000, 70_001))
    if kind in ("n_lower", "twin", "two_letter"):
        return int(rng.integers(max(300, k + 120), max(1500, 2 * k + 400)))
    return int(rng.choice([int(rng.integers(40, 301)), int(rng.integers(300, 1201)), int(rng.integers(1200, 3001))]))  # spread


def _plan(rng, k, kinds, lens):
    """which reference every planted copy comes from.  Slots: 0 - 2 the copies across the first three chunk cuts, 3 - 8 the OPS of the
    main contig, 9 / 10 the copies at the first and the last base of the edge contig, 11 the sequences of 3 .. 2k + 1 bases, 12 the one
    with Ns, 13 / 14 the long contigs.  -> (sources, True when the reverse-complemented copy's reference has no other copy in its contig)"""
    ok = [r for r in range(len(kinds)) if lens[r] >= k + 20]
    if not ok:
        ok = [int(np.argmax(lens))]
    src = [int(rng.choice(ok)) for _ in range(15)]
    longs = [r for r in range(len(kinds)) if kinds[r] == "long"]
    for slot, r in zip((4, 3, 13), longs + longs):  # every long reference has a copy in the main contig
        src[slot] = r
    twin = [r for r in range(len(kinds)) if kinds[r] == "twin"]
    same = lambda a, b: a == b or (a in twin and b in twin)
    others = [r for r in ok if not any(same(r, src[s]) for s in range(8))]
    alone = bool(others)
    if alone:
        src[8] = int(rng.choice(others))
    return tuple(src), alone


def config(seed):
    """everything one iteration draws, from `seed` alone"""
    rng = np.random.default_rng([0x72736574, int(seed)])
    cls = K_CLASSES[int(rng.integers(0, len(K_CLASSES)))]
    k = int(rng.choice(cls, p=[0.1, 0.15, 0.3, 0.45])) if cls is K_CLASSES[0] else int(rng.choice(cls))  # (k = 1: nothing but a refusal)
    rc = bool(rng.random() < 0.4)
    n_refs = int(rng.choice([3, 4, 6, 9, 12, 16, 20, 24]))
    kinds = [n for n in KINDS if rng.random() < KIND_P[n] and not (n == "short" and k == 1)]
    n_long = int(rng.choice([0, 1, 2], p=[0.5, 0.25, 0.25])) if k >= LONG_MIN_K else 0
    kinds = kinds + ["twin"] * ("twin" in kinds) + ["long"] * n_long
    kinds = [kinds[i] for i in rng.permutation(len(kinds))][:n_refs]
    if kinds.count("twin") == 1:
        kinds[kinds.index("twin")] = "spread"
    kinds += ["spread"] * (n_refs - len(kinds))
    kinds = [kinds[i] for i in rng.permutation(n_refs)]  # the drawn order: the kinds alternate inside the slabs
    lens = [_ref_len(rng, n, k) for n in kinds]
    tw = [r for r, n in enumerate(kinds) if n == "twin"]
    if tw:
        lens[tw[1]] = lens[tw[0]]
    find_prob_half = bool(rng.random() < 0.15)
    if find_prob_half and rng.random() < 0.7:  # (fewer than 11 k-mers: the threshold at 0.5 is 1 and every call refuses the set)
        for r, n in enumerate(kinds):
            if n in ("k", "k1"):
                kinds[r], lens[r] = "spread", _ref_len(rng, "spread", k)
    # rows of a long reference: about a row a base, twice that with add_revcomp
    rows = sorted((lens[r] + 1) * (2 if rc else 1) for r, n in enumerate(kinds) if n == "long")
    long_route, wide_rows = "none", int(rng.choice([MAX_ROWS, 1 << 17, WIDE_MAX_ROWS]))
    if rows:
        long_route = "index" if rng.random() < 0.28 else "wide"
        if long_route == "wide":
            wide_rows = int(rng.choice([min(WIDE_MAX_ROWS, rows[-1] + 4096), WIDE_MAX_ROWS]))
        else:  # the largest one above max_wide_rows, a second one below it
            wide_rows = MAX_ROWS if len(rows) == 1 or rows[0] + 2048 > rows[-1] - 2048 else int((rows[0] + rows[-1]) // 2)
    prefilter, positions = bool(rng.random() < 0.6), bool(rng.random() < 0.6)
    legs = {n: bool(rng.random() < LEG_P[n]) for n in LEGS}
    shape = str(rng.choice(["one", "base", "base", "base", "base", "below64", "above64", "above64", "many"]))
    n_seqs = {"one": 1, "base": 9, "below64": int(rng.integers(40, 64)), "above64": int(rng.integers(64, 91)),
              "many": int(rng.integers(100, 301))}[shape]
    many_chunks = bool(k >= LONG_MIN_K and n_seqs > 1 and rng.random() < 0.13)
    huge = bool(k >= LONG_MIN_K and n_seqs > 1 and rng.random() < 0.06)
    n_seqs = max(n_seqs, 9 + many_chunks + huge) if n_seqs > 1 else 1
    sources, alone = _plan(rng, k, kinds, lens)
    order = tuple(int(x) for x in rng.permutation(n_seqs))
    n_short = int(rng.integers(1, 5)) if rng.random() < 0.5 else 0
    short_seqs = tuple(sorted((int(rng.integers(0, n_seqs + 1)), int(rng.integers(0, 3))) for _ in range(n_short)))
    p_err = float(rng.choice([1e-7, 1e-4]))
    if many_chunks and k >= 130 and p_err == 1e-4:
        # 258 chunks of 4k bases are a quarter of a million random bases, and at 1e-4 the references of k and k + 1 bases have thresholds
        # of 6 and 7: thousands of sites that only cost time.  The slot is a filler then (make_inputs fills the batch up to n_seqs)
        many_chunks = False
    return Config(seed=int(seed), k=k, add_revcomp=rc, kinds=tuple(kinds), ref_lens=tuple(lens), wide_rows=wide_rows, long_route=long_route,
                  prefilter=prefilter, positions=positions, n_seqs=n_seqs, many_chunks=many_chunks, huge=huge, sources=sources, order=order,
                  short_seqs=short_seqs, max_error_prob=p_err, find_prob=0.5 if find_prob_half else p_err,
                  max_gap_len=int(rng.choice([0, 5, 40])), strands=int(rng.choice([1, 2, 3, 3])),
                  slab_bytes=int(rng.choice([1 << 16, 1 << 18, 16 << 20])), record_capacity=int(rng.choice([1, 1 << 16], p=[0.3, 0.7])),
                  refs_per_slab=int(rng.choice([0, 1, 3])), caps=str(rng.choice(["ample", "ample", "pairs", "bases"])),
                  capacity=str(rng.choice(["ample", "exact", "below"])), max_sites=str(rng.choice(["ample", "ample", "below"])),
                  call_add_revcomp=bool(k >= 32 and alone and p_err == 1e-7 and "two_letter" not in kinds and rng.random() < 0.7), legs=legs)


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _mutate(rng, a, rate):
    a = a.copy()
    pos = np.flatnonzero((rng.random(len(a)) < rate) & np.isin(a, ACGT))
    a[pos] = ACGT[(np.searchsorted(ACGT, a[pos]) + rng.integers(1, 4, len(pos))) % 4]
    return a


def make_refs(cfg):
    rng = np.random.default_rng([0x72736574, int(cfg.seed), 1])
    refs, twin = [], None
    for kind, n in zip(cfg.kinds, cfg.ref_lens):
        a = _rnd(rng, n)
        if kind == "n_lower":  # an N and a lower-case stretch: no bases, on either strand
            a[n // 3] = ord("N")
            a[n // 2:n // 2 + 20] |= 0x20
        elif kind == "two_letter":  # deep LCS structure, long scans
            a = ACGT[[0, 3]][rng.integers(0, 2, n)].copy()
        elif kind == "twin":
            if twin is None:
                twin = a
            a = twin.copy()
        refs.append(a)
    return refs


def _piece(rng, ref, k, most=None):
    """(a, w): a stretch of ref to plant - 2k + 40 bases or 300, whichever is more, or all of it"""
    w = min(len(ref), max(2 * k + 40, 300) if most is None else most)
    a = int(rng.integers(0, len(ref) - w + 1))
    return a, w


def make_inputs(cfg):
    """-> (refs, seqs, planted): the references, the sequences of the host batch (all of 3 bases or more) in their drawn order, and the
    planted copies as dicts(seq, at, ref, a, w, op[, x]): seqs[seq][at:...] is ref[a:a + w] after `op` (x: where an indel lies)"""
    refs = make_refs(cfg)
    rng = np.random.default_rng([0x72736574, int(cfg.seed), 2])
    k, chunk, src = cfg.k, chunk_of(cfg.k), cfg.sources
    planted = []

    def put(s, contig, at, r, op, most=None):
        a, w = _piece(rng, refs[r], k, most)
        p = refs[r][a:a + w]
        rec = dict(seq=s, at=at, ref=r, a=a, w=w, op=op)
        if op == "sub1":
            p = _mutate(rng, p, 0.01)
        elif op == "sub3":
            p = _mutate(rng, p, 0.03)
        elif op == "rc":
            p = revcomp(p)
        elif op in ("ins2", "del3") and w > 12:
            rec["x"] = x = int(rng.integers(4, w - 7))
            p = np.concatenate([p[:x], _rnd(rng, 2), p[x:]]) if op == "ins2" else np.concatenate([p[:x], p[x + 3:]])
        elif op in ("ins2", "del3"):
            rec["op"] = "exact"
        contig[at:at + len(p)] = p
        planted.append(rec)
        return len(p)

    slot = max(2 * k + 40, 300) + 100
    main = _rnd(rng, 3 * chunk + 100 + 6 * slot + 50)
    for i in range(3):  # across the first three multiples of the chunk
        put(0, main, (i + 1) * chunk - 75, src[i], "exact", most=150)
    for i, op in enumerate(OPS):
        put(0, main, 3 * chunk + 100 + i * slot, src[3 + i], op)
    seqs = [main]
    if cfg.n_seqs > 1:
        a0, w0 = _piece(rng, refs[src[9]], k)
        a1, w1 = _piece(rng, refs[src[10]], k)
        edge = _rnd(rng, w0 + 200 + w1)
        edge[:w0] = refs[src[9]][a0:a0 + w0]          # from the contig's first base
        edge[w0 + 200:] = refs[src[10]][a1:a1 + w1]   # to its last
        planted.append(dict(seq=1, at=0, ref=src[9], a=a0, w=w0, op="exact"))
        planted.append(dict(seq=1, at=w0 + 200, ref=src[10], a=a1, w=w1, op="exact"))
        seqs.append(edge)
        r = refs[src[11]]
        for n in (3, k - 1, k, k + 1, 2 * k + 1):
            n = max(3, n)
            seqs.append(r[:n].copy() if len(r) >= n else _rnd(rng, n))
        a, w = _piece(rng, refs[src[12]], k)
        with_n = np.concatenate([_rnd(rng, 60), _mutate(rng, refs[src[12]][a:a + w], 0.01), _rnd(rng, 40)])
        with_n[[60 + w // 4, 61 + w // 4, 60 + (3 * w) // 4]] = ord("N")
        seqs += [with_n, _rnd(rng, 500)]  # the one with Ns, the unrelated one
        if cfg.many_chunks:  # more than 256 chunks: a second task per reference
            big = _rnd(rng, TASK_ITEMS * chunk + 2 * chunk + 7)
            put(len(seqs), big, TASK_ITEMS * chunk - 100, src[13], "exact")
            put(len(seqs), big, 5 * chunk + 31, src[14], "sub1")
            seqs.append(big)
        if cfg.huge:  # more than 65 536 bases, a copy across that position
            big = _rnd(rng, 65536 + 3000)
            put(len(seqs), big, 65536 - 120, src[14], "exact")
            put(len(seqs), big, 40_000, src[13], "sub1")
            seqs.append(big)
        while len(seqs) < cfg.n_seqs:  # fillers: short slices of references and random bases
            n = int(rng.integers(5, 121))
            r = refs[int(rng.integers(0, len(refs)))]
            if rng.random() < 0.5 and len(r) > n:
                a = int(rng.integers(0, len(r) - n + 1))
                seqs.append(r[a:a + n].copy())
            else:
                seqs.append(_rnd(rng, n))
    assert len(seqs) == cfg.n_seqs
    where = np.argsort(np.asarray(cfg.order))  # sequence i of the list above is sequence where[i] of the batch
    for rec in planted:
        rec["seq"] = int(where[rec["seq"]])
    return refs, [np.ascontiguousarray(seqs[i], dtype=np.uint8) for i in cfg.order], planted


def with_shorts(cfg, seqs):
    """the batch of the device legs: cfg.short_seqs put in -> (sequences, index in it of every sequence of the host batch)"""
    out, index, at = [], [], 0
    for where, n in list(cfg.short_seqs) + [(len(seqs), -1)]:
        for s in range(at, where):
            index.append(len(out))
            out.append(seqs[s])
        at = where
        if n >= 0:
            out.append(ACGT[(np.arange(n) + where) % 4].copy())
    return out, np.asarray(index, dtype=np.int64)


# The suite's fixed list (the two test modules run exactly these; tools/stress.py with SOAK=refset draws seeds beyond it).
SEEDS = tuple(range(1, 161))
STRESS_FIRST_SEED = 100_000
