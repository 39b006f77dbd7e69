"""The generator of the third randomized oracle soak, over positions, segments, depth, placement, pileup and indels (imported by
tests/test_locate_random_configs_host.py, tests/test_gpu_locate_random_configs.py and tools/stress.py; holds no test itself).
config(seed) draws everything one iteration checks - k by class, the sources and how their index and its position table are made, the
batch's shape and its edits, bridge, strands and their order, skip_multi, the site thresholds, max_gap / max_indel, merge and the
capacities of d_segs and d_sites; from a stream of its own the indel calls' max_indel, thresholds and the capacities of d_events and
their d_sites - and make_inputs(cfg) makes the bytes.  Pure numpy: no GPU, no product library, no oracle; the same
seed gives the same bytes on any machine.

What the draws are for (kbo_amd/csrc/locate_kernels.hip, place_kernels.hip, pileup_kernels.hip): a tile of TILE positions looks HALO
beyond either end, so sequences of m * TILE +- 1 and TILE + HALO +- 1 bases put a segment's start and end into different tiles;
tile_sequences strides over the sequence starts inside a tile 256 at a time; a list of more than LANE_MAX segments leaves the lane for
a wave, one of more than WINDOW wraps the wave's ring; pileup_kernel takes a record's windows 64 at a time and carries a gap across
rounds.  K_CLASSES is tests/random_configs.py's without k = 1 and 2: nothing but refusals."""
from dataclasses import dataclass

import numpy as np

from random_configs import ACGT

# {3, 5}, {8 .. 31}, {32, 33}, {47 .. 63}, {64, 65}, {66 .. 127}, {128, 129}, {130 .. 254}, {255}
K_CLASSES = ((3, 5), tuple(range(8, 32)), (32, 33), tuple(range(47, 64)), (64, 65), tuple(range(66, 128)), (128, 129), tuple(range(130, 255)), (255,))
TILE, HALO = 2048, 256        # kbo_segments_geometry (the test modules compare)
LANE_MAX, WINDOW = 4, 64      # KBO_PLACE_LANE_MAX, KBO_PLACE_WINDOW
STARTS_TURN = 256             # tile_sequences: sequence starts a turn
SHAPES = ("reads", "tiny", "long", "junction", "mixed")
HOWS = ("host", "device", "parts")
CAPS = ("ample", "exact", "below", "zero")
COMP = np.arange(256, dtype=np.uint8)  # (lower case stays what it is: no base on either strand)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


def k_class(k):
    return next(i for i, c in enumerate(K_CLASSES) if k in c)


def revcomp(a):
    return COMP[a[::-1]]


def capacity(mode, n):
    return {"ample": n + 9, "exact": n, "below": max(0, n - 1 - n // 3), "zero": 0}[mode]


@dataclass
class Config:
    seed: int
    k: int
    add_revcomp: bool
    src_lens: tuple            # of every source, in order; the longest holds the planted repeats
    how: str                   # the index: built on the host, on the device, or from_parts
    slab: int                  # kbo_set_positions_slab_bases: 0, fewer than k + 1, or a mid value
    shape: str
    sub_rate: float            # 0, 0.01 or 0.05
    bridge: int
    strands: tuple             # the calls, in order: (1,), (2,), (1, 2) or (2, 1)
    skip_multi: bool
    min_count: int
    frac_num: int
    frac_den: int
    max_gap: int
    max_indel: int
    merge: bool                # the second strand's kbo_place_dev merges into the first's records (else it writes over them)
    seg_cap: str               # of d_segs, every strand: CAPS
    site_cap: str              # of d_sites: CAPS
    ev_max_indel: int          # kbo_indels_dev's own max_indel (cfg.max_indel is placement's and may be 0, which the events refuse)
    ev_min_count: int          # the indel sites' thresholds
    ev_frac_num: int
    ev_frac_den: int
    event_cap: str             # of d_events, the list of every strand: CAPS
    ev_site_cap: str           # of the indel d_sites: CAPS

    def describe(self):
        return ("seed=%d k=%d rc=%s srcs=%d (%d bases) how=%s slab=%d shape=%s subs=%g bridge=%d strands=%s skip_multi=%s sites=%d,%d/%d "
                "max_gap=%d max_indel=%d merge=%s seg_cap=%s site_cap=%s events: max_indel=%d sites=%d,%d/%d event_cap=%s site_cap=%s"
                % (self.seed, self.k, self.add_revcomp, len(self.src_lens), sum(self.src_lens), self.how, self.slab, self.shape, self.sub_rate,
                   self.bridge, self.strands, self.skip_multi, self.min_count, self.frac_num, self.frac_den, self.max_gap, self.max_indel,
                   self.merge, self.seg_cap, self.site_cap, self.ev_max_indel, self.ev_min_count, self.ev_frac_num, self.ev_frac_den, self.event_cap,
                   self.ev_site_cap))


def config(seed):
    """everything one iteration draws, from `seed` alone"""
    rng = np.random.default_rng([0x6C6F6361, int(seed)])
    cls = K_CLASSES[int(rng.integers(0, len(K_CLASSES)))]
    k = int(rng.choice(cls))
    # the first source holds the planted repeats (6 stretches of up to k + 30 bases) and gives the long sequences their text
    total = int(rng.choice([2000, 6000, 12000, 30000], p=[0.2, 0.3, 0.3, 0.2]))
    if k >= 128:
        total = min(total, 12000)  # (the oracle spells every row's k-mer, the brute force hashes every window: both grow with k)
    n_srcs = int(rng.choice([1, 2, 3, 5, 8, 12, 20, 40]))
    small = [int(rng.choice([0, 0, 1, k - 1, k, k + 5, int(rng.integers(64, 401))])) for _ in range(n_srcs - 1)]
    second = int(rng.integers(max(2 * k + 60, 300), max(2 * k + 61, total // 3))) if n_srcs > 1 and total >= 6000 else None
    if second is not None:
        small[int(rng.integers(0, len(small)))] = second
    main = max(total - sum(small), 16 * k + 400, 1500)
    where = int(rng.integers(0, n_srcs))  # sources in front of the long one too: its coordinates do not start at 0
    lens = small[:where] + [main] + small[where:]
    bridge = int(rng.choice([0, 1, k - 1, k, k, min(k + 1, 255), 255, 255, int(rng.integers(0, 256))]))
    ev = np.random.default_rng([0x6C6F6361, int(seed), 3])  # the indel calls' fields from a stream of their own: every field above keeps its value
    indel = dict(ev_max_indel=int(ev.choice([1, 5, 16, 17, 100, 0xFFFFFFFF])), ev_min_count=int(ev.choice([1, 1, 2, 3])), ev_frac_num=int(ev.choice([0, 1, 1, 2])),
                 ev_frac_den=int(ev.choice([1, 2, 3])), event_cap=str(ev.choice(CAPS, p=[0.4, 0.25, 0.25, 0.1])),
                 ev_site_cap=str(ev.choice(CAPS, p=[0.4, 0.25, 0.25, 0.1])))
    return Config(seed=int(seed), k=k, add_revcomp=bool(rng.random() < 0.5), src_lens=tuple(lens), how=str(rng.choice(HOWS)),
                  slab=int(rng.choice([0, int(rng.integers(1, k + 1)), int(rng.integers(k + 1, 2000))])), shape=str(rng.choice(SHAPES)),
                  sub_rate=float(rng.choice([0.0, 0.01, 0.05])), bridge=bridge, strands=((1,), (2,), (1, 2), (2, 1))[int(rng.integers(0, 4))],
                  skip_multi=bool(rng.random() < 0.5), min_count=int(rng.choice([1, 1, 2, 3])), frac_num=int(rng.choice([0, 1, 1, 2])),
                  frac_den=int(rng.choice([1, 2, 3])), max_gap=int(rng.choice([0, 50, 1000, 1000])), max_indel=int(rng.choice([0, 5, 100, 100])),
                  merge=bool(rng.random() < 0.7), seg_cap=str(rng.choice(CAPS, p=[0.4, 0.25, 0.25, 0.1])),
                  site_cap=str(rng.choice(CAPS, p=[0.4, 0.25, 0.25, 0.1])), **indel)


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def main_source(cfg):
    return int(np.argmax(cfg.src_lens))


def make_sources(cfg):
    """the sources: random text; in the longest one an exact repeat of k + 20 bases (MULTI), an inverted repeat of k + 10, a tandem
    repeat of a unit of 7 over k + 30 bases, an N and a lower-case base; a second inverted repeat from the longest into the second
    longest"""
    rng = np.random.default_rng([0x6C6F6361, int(cfg.seed), 1])
    k = cfg.k
    srcs = [_rnd(rng, n) for n in cfg.src_lens]
    m = srcs[main_source(cfg)]
    step = (len(m) - (k + 40)) // 7  # seven slots of at least 2k + 40 bases (the longest source has 16k + 400)
    assert step >= 2 * k + 40
    m[2 * step:2 * step + k + 20] = m[0:k + 20]
    m[3 * step:3 * step + k + 10] = revcomp(m[step:step + k + 10])
    m[4 * step:4 * step + k + 30] = np.resize(m[4 * step:4 * step + 7], k + 30)
    m[5 * step + 5] = ord("N")
    m[6 * step + 9] |= 0x20
    big = [i for i in np.argsort(cfg.src_lens)[::-1][1:2] if cfg.src_lens[i] >= k + 40]
    for i in big:
        srcs[i][10:10 + k + 10] = revcomp(m[step + k + 20:step + 2 * k + 30])
    return srcs


def _edit(rng, q, cfg, dense=False):
    """substitutions at the configuration's rate, one time in four an insertion or a deletion of 1 .. 20 bases, one time in ten an N;
    dense: a substitution every max(2, k // 2) bases over the middle 70 .. 120 bases - no window there matches, the diagonal holds"""
    q = q.copy()
    pos = np.flatnonzero((rng.random(len(q)) < cfg.sub_rate) & np.isin(q, ACGT))
    q[pos] = ACGT[(np.searchsorted(ACGT, q[pos]) + rng.integers(1, 4, len(pos))) % 4]
    if dense:
        span = int(rng.integers(70, 121))
        a = (len(q) - span) // 2
        pos = np.arange(a, a + span, max(2, cfg.k // 2))
        pos = pos[np.isin(q[pos], ACGT)]
        q[pos] = ACGT[(np.searchsorted(ACGT, q[pos]) + 1) % 4]
        return q
    if len(q) > 40 and rng.random() < 0.25:
        x, n = int(rng.integers(10, len(q) - 10)), int(rng.integers(1, 21))
        q = np.concatenate([q[:x], _rnd(rng, n), q[x:]]) if rng.random() < 0.5 else np.concatenate([q[:x], q[x + n:]])
    if len(q) and rng.random() < 0.1:
        q[int(rng.integers(0, len(q)))] = ord("N")
    return q


def make_inputs(cfg):
    """-> (sources, sequences of the batch)"""
    srcs = make_sources(cfg)
    rng = np.random.default_rng([0x6C6F6361, int(cfg.seed), 2])
    k = cfg.k
    cat = np.concatenate(srcs)
    soff = np.concatenate([[0], np.cumsum(cfg.src_lens)])
    m0, m1 = int(soff[main_source(cfg)]), int(soff[main_source(cfg) + 1])

    def piece(n, anywhere=False):
        """n bases of the longest source (anywhere: of the sources as they follow each other), either strand"""
        lo, hi = (0, len(cat)) if anywhere else (m0, m1)
        n = min(n, hi - lo)
        a = int(rng.integers(lo, hi - n + 1))
        return cat[a:a + n]

    kept = []

    def read(n, dense=False):
        if kept and n > 20 and rng.random() < 0.3:  # the same read again: a bridged base counted more than once
            return kept[int(rng.integers(0, len(kept)))]
        q = _edit(rng, piece(n, anywhere=rng.random() < 0.2), cfg, dense)
        q = revcomp(q) if rng.random() < 0.5 else q
        if n > 20:
            kept.append(q)
        return q

    def text(n):
        """a sequence of exactly n bases: stretches of the longest source one behind the other, a substitution between them"""
        out = []
        while sum(len(p) for p in out) < n:
            out.append(_edit(rng, piece(min(m1 - m0, n)), cfg)[:n - sum(len(p) for p in out)])
        return np.concatenate(out)[:n]

    read_len = (lambda: int(rng.integers(100, 161))) if k <= 100 else (lambda: k + int(rng.integers(20, 101)))  # (a read shorter than k holds no window)
    reads = lambda n: [read(read_len()) for _ in range(min(n, max(5, 12000 // (k + 60))))]  # noqa: E731 (the brute force's cost grows with k x bases)
    dense = lambda n: [read(2 * k + 140, dense=True) for _ in range(n)]  # noqa: E731

    def tiny(most_bases, most_seqs):
        out, total = [], 0
        while total < most_bases and len(out) < most_seqs:
            n = int(rng.integers(k - 1, 2 * k + 1)) if rng.random() < min(0.1, 2.0 / k) else int(rng.integers(0, 10))  # (fewer than 10 bases a sequence on average)
            out.append(read(n) if n else np.zeros(0, dtype=np.uint8))
            total += len(out[-1])
        return out

    def snp_reads(n):
        """n reads over one base of the longest source, k + 1 .. k + 40 bases to either side of it, four in five with the same
        substitution there: bridged when bridge >= k, a column that counts up to n"""
        at = int(rng.integers(m0 + k + 45, m1 - k - 45))
        alt = ACGT[(int(np.searchsorted(ACGT, cat[at])) + 1) % 4] if cat[at] in ACGT else ACGT[0]
        out = []
        for _ in range(n):
            a, b = int(rng.integers(k + 1, k + 41)), int(rng.integers(k + 1, k + 41))
            q = cat[at - a:at + b].copy()
            if rng.random() < 0.8:
                q[a] = alt
            out.append(revcomp(q) if rng.random() < 0.5 else q)
        return out

    def junctions(n):
        nonempty = [j for j in range(1, len(srcs)) if cfg.src_lens[j] and soff[j] > 0]
        out = []
        for _ in range(n if nonempty else 0):
            j = int(soff[nonempty[int(rng.integers(0, len(nonempty)))]])
            a, b = int(rng.integers(k // 2 + 1, k + 60)), int(rng.integers(k // 2 + 1, k + 60))
            out.append(_edit(rng, cat[max(0, j - a):j + b], cfg))
        return out

    def indel_reads(n):
        """n reads over one place of the longest source, k + 1 .. k + 40 bases to either side of it, four in five with the same insertion
        or deletion of 1 .. 20 bases there, on either strand: two segments and one event a read, a site that counts up to n.  From a
        generator of their own and behind everything else: no other sequence of any seed changes"""
        own = np.random.default_rng([0x6C6F6361, int(cfg.seed), 4])
        at, ln = int(own.integers(m0 + k + 45, m1 - k - 65)), int(own.integers(1, 21))
        ins = _rnd(own, ln) if own.random() < 0.5 else None
        out = []
        for _ in range(n):
            a, b = int(own.integers(k + 1, k + 41)), int(own.integers(k + 1, k + 41))
            if own.random() >= 0.8:
                q = cat[at - a:at + b].copy()
            elif ins is not None:
                q = np.concatenate([cat[at - a:at], ins, cat[at:at + b]])
            else:
                q = np.concatenate([cat[at - a:at], cat[at + ln:at + ln + b]])
            out.append(revcomp(q) if own.random() < 0.5 else q)
        return out

    if cfg.shape == "reads":
        seqs = reads(int(rng.integers(60, 201))) + dense(2) + snp_reads(8)
    elif cfg.shape == "tiny":
        seqs = [np.zeros(0, dtype=np.uint8)] + tiny(20000, 4000) + reads(10) + snp_reads(6) + [np.zeros(0, dtype=np.uint8)]
    elif cfg.shape == "long":
        lens = [TILE + HALO + 1, TILE - 1, TILE + HALO - 1, TILE + 1, 2 * TILE + 1, 2 * TILE - 1]
        seqs = [text(n) for n in [lens[i] for i in rng.permutation(len(lens))[:int(rng.integers(3, 7)) if k < 128 else 3]]] + dense(2) + reads(5) + snp_reads(8)
    elif cfg.shape == "junction":
        seqs = junctions(40) + reads(40) + dense(1) + snp_reads(8)
    else:
        seqs = reads(30) + tiny(3000, 700) + [text(TILE + HALO + 1)] + junctions(10) + dense(2) + snp_reads(8)
        seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    seqs = seqs + indel_reads(6 if cfg.shape == "tiny" else 8) + ([np.zeros(0, dtype=np.uint8)] if cfg.shape == "tiny" else [])  # (tiny ends with an empty sequence)
    return srcs, [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]


# The suite's fixed list (the two test modules run exactly these; tools/stress.py with SOAK=locate draws seeds beyond it).
SEEDS = tuple(range(1, 78))
STRESS_FIRST_SEED = 100_000
