"""The randomized oracle soak's generator (imported by tests/test_gpu_random_configs.py, tests/test_random_configs_host.py and
tools/stress.py; holds no test itself).  config(seed) draws everything one iteration checks - k, index content, every process-wide
knob, the batch's shape and lengths, error rates, which optional legs run - and make_inputs(cfg) makes the bytes.  Pure numpy: no
GPU, no product library, no oracle; the same seed gives the same bytes on any machine.

k is drawn by class (K_CLASSES) so that every key width and every kernel boundary gets its share; read lengths at the one kernel's
boundaries (BOUNDARY_READ_LENS, reads shorter than k / the threshold) and sequence lengths around map_long_kernel's piece size
(long_boundary_lens) are drawn on purpose."""
from dataclasses import dataclass, field

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# {1, 2, 3, 5}, {8 .. 31}, {32, 33}, {47 .. 63}, {64, 65}, {66 .. 127}, {128, 129}, {130 .. 254}, {255}
K_CLASSES = ((1, 2, 3, 5), tuple(range(8, 32)), (32, 33), tuple(range(47, 64)), (64, 65), tuple(range(66, 128)), (128, 129),
             tuple(range(130, 255)), (255,))
GENOMES = (2_000, 30_000, 200_000)
# map_reads_kernel takes reads of at most 160 bases in words of 16 positions
BOUNDARY_READ_LENS = (3, 4, 15, 16, 17, 31, 32, 33, 48, 64, 96, 128, 144, 159, 160, 161)
LONG_REGION = 1008  # kernels.hpp kLongRegion: the bases a piece of map_long_kernel holds, 2k + 1 of them warm-up
LEGS = ("packed", "find", "device", "call", "devbuild", "map_opts", "fill_gaps", "sparse", "stream", "shards")
# probability of each optional leg (a is always run): a seed decides, not the clock
LEG_P = {"packed": 0.4, "find": 0.5, "device": 0.9, "call": 0.3, "devbuild": 0.2, "map_opts": 0.3, "fill_gaps": 0.35, "sparse": 0.4,
         "stream": 0.4, "shards": 0.25}
# the second set of legs (l - q of the GPU module), drawn into Config.extra from a stream of their own (_extra): entry points added
# after the first set, which take map_reads_kernel / finish_reads_kernel through their summary and run-count forms, double a slab on
# the device for the other strand, or take a real walk's MS bytes and characters at a threshold per sequence
LEGS2 = ("summary", "strands", "find_dev", "seq_thresholds", "rle_dev", "revcomp_dev")
LEG2_P = {"summary": 0.6, "strands": 0.55, "find_dev": 0.6, "seq_thresholds": 0.5, "rle_dev": 0.5, "revcomp_dev": 0.5}
SUMMARY_FORMS = ("host", "packed", "device", "stream")
# kbo_derand_*_seq_dev: what a sequence's threshold is drawn from, t the oracle's threshold of the index (resolved by thresholds_of)
N_THR_CANDIDATES = 7
COMP = np.arange(256, dtype=np.uint8)  # kbo_hip.h "both strands": A <-> T, C <-> G, a <-> t, c <-> g, every other byte unchanged
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def k_class(k):
    return next(i for i, c in enumerate(K_CLASSES) if k in c)


def long_own(k):
    """the bases of its own a piece of map_long_kernel maps (long_kernels.hip: (kLongRegion - 2k - 1) & ~15)"""
    return (LONG_REGION - 2 * k - 1) & ~15


def long_boundary_lens(k):
    own = long_own(k)  # (2k + 1 + kLongOwnMin <= kLongRegion up to k = 375)
    out = [own - 1, own, own + 1, 2 * own, 2 * own + 1, LONG_REGION - 16, LONG_REGION, LONG_REGION + 16]
    if k >= 64:
        out += [k - 1, k, k + 1, 2 * k, 2 * k + 1]
    return [n for n in out if n >= 3]


@dataclass
class Config:
    seed: int
    k: int
    G: int                     # bases of the genome before repeats are appended
    genome_seed: int
    repeats: bool              # tandem repeats, one non-ACGT byte and a reversed stretch appended to the index text
    n_contigs: int             # the index text cut into this many contigs ...
    short_contigs: int         # ... plus this many contigs shorter than k
    add_revcomp: bool
    knobs: dict                # process-wide settings, see apply_knobs() of the GPU module
    shape: str
    lens: tuple                # the main batch: one length per sequence
    short_seqs: tuple          # (where, length 0 / 1 / 2): sequences the device entry points take inside a batch (kbo_hip.h: no alignment for
                               # them, every other sequence as without them) and kbo_ms_batch takes unless empty: with_shorts()
    refuse_len: int            # -1, or 0 / 1 / 2: a sequence of that length put into the main batch at refuse_at, which the host entry points
    refuse_at: int             # refuse as a whole (kbo_hip.h KBO_E_EMPTY_QUERY, KBO_E_LEN_LE_2); the legs then run without it
    sub_rate: float
    indel: bool
    n_bytes: bool
    max_error_prob: float
    gap_len: int               # kbo::find's max_gap_len
    packed_gap_len: int
    legs: dict                 # leg name -> bool
    call_emit: int             # kbo_set_call_device_emit
    call_pick: tuple
    map_opts: tuple            # (fill_gaps, call_variants, format) of leg g
    opts_lens: tuple           # legs g / h: lengths of the sequences with substituted blocks; edge lengths are appended by make_inputs
    dev_format: bool
    dev_zero_sizing: bool      # DeviceBatch with work memory sized for max_len = 0
    tail_stream: bool
    stream_pipelines: int
    stream_parts: int
    shards: int
    extra: dict = field(default_factory=dict)

    def describe(self):
        return ("seed=%d k=%d G=%d rc=%s contigs=%d+%d repeats=%s shape=%s n=%d max_len=%d sub=%g p=%g knobs=%s legs=%s"
                % (self.seed, self.k, self.G, self.add_revcomp, self.n_contigs, self.short_contigs, self.repeats, self.shape,
                   len(self.lens), max(self.lens), self.sub_rate, self.max_error_prob, self.knobs,
                   [n for n in LEGS if self.legs[n]] + [n for n in LEGS2 if self.extra.get("legs", {}).get(n)]))


def _knobs(rng):
    """the soak's knob draws; four configurations in ten keep the plan / depth-table / guided-walk knobs as shipped, so that the
    routes users take (the one-kernel routes, which many corners switch off) get their share of the list next to the corners"""
    kn = {"pair_steps": (0 if rng.random() < 0.5 else (1 << 63), int(rng.choice([1, 4, 16]))),
          "slab_bytes": int(rng.choice([1 << 16, 1 << 18, 32 << 20])),
          "big_layout": bool(rng.random() < 0.15),
          "two_workers": bool(rng.random() < 0.15)}
    corners = bool(rng.random() < 0.6)
    draws = {"plan": (int(rng.random() < 0.75), int(rng.choice([-1, 1, 4, 10, 14, 20])), int(rng.choice([4, 16, 40, 64]))),
             "plan_tuning": (int(rng.choice([-1, 2, 3, 8, 20, 40])), int(rng.choice([16, 32, 100])),
                             int(rng.choice([0, 8, 32, 50, 64, 0xFFFF]))),
             "unit_cap_divisor": int(rng.choice([1, 1, 1, 4, 30])),
             "guided_walk": (int(rng.choice([0, 1, 8, 32])), int(rng.choice([-1, 0, 1]))),
             "depth_table": int(rng.choice([0, 0, -1, 1, 1, 3, 6, 9, 12, 16, 16])),
             "depth_table_anchors": int(rng.choice([-1, 0, 1, 1]))}
    shipped = {"plan": (1, -1, 64), "plan_tuning": (-1, 32, 50), "unit_cap_divisor": 1, "guided_walk": (0, -1), "depth_table": 0,
               "depth_table_anchors": -1}
    kn.update(draws if corners else shipped)  # (drawn either way: the later draws do not depend on `corners`)
    kn["corners"] = corners
    return kn


def _lens(rng, k, shape, glen):
    lens = []
    if shape in ("uniform", "mixed"):
        lens += [int(rng.choice([32, 100, 128, 150, 151, 250, 256, 480]))] * int(rng.integers(50, 800))
    if shape in ("ragged", "mixed"):
        lens += [int(x) for x in rng.integers(3, 600, int(rng.integers(50, 800)))]
    if shape == "reads":  # what the one kernel takes: at most 160 bases
        lens += [int(x) for x in rng.integers(3, 161, int(rng.integers(50, 1500)))]
    if shape == "reads_uniform":
        lens += [int(rng.choice([32, 100, 128, 150, 159, 160]))] * int(rng.integers(50, 1500))
    if shape == "reads_boundary":  # every boundary length of map_reads_kernel except 161, reads shorter than k and than any threshold
        lens += [n for n in BOUNDARY_READ_LENS if n <= 160] * int(rng.integers(2, 20))
        lens += [int(x) for x in rng.integers(3, 161, int(rng.integers(20, 400)))]
        lens += [n for n in (k - 1, k, k + 1) if 3 <= n <= 160]
    if shape == "ragged_boundary":  # as above with 161: one base too many for the one kernel
        lens += list(BOUNDARY_READ_LENS) * int(rng.integers(2, 10))
        lens += [int(x) for x in rng.integers(3, 200, int(rng.integers(20, 400)))]
    if shape in ("long", "mixed"):
        lens += [int(x) for x in rng.integers(481, 30_000, int(rng.integers(1, 12)))]
    if shape == "long_boundary":  # around map_long_kernel's piece size, and around k for large k
        lens += long_boundary_lens(k) * int(rng.integers(1, 4))
        lens += [int(x) for x in rng.integers(161, 5000, int(rng.integers(5, 60)))]
    lens = [max(3, min(n, glen - 1)) for n in lens]  # (a sequence of 0, 1 or 2 bases makes the host entry points refuse the batch: refuse_len)
    order = rng.permutation(len(lens))
    return tuple(lens[i] for i in order)


def _extra(seed, k, knobs, lens, short_seqs):
    """Config.extra: the draws of legs l - q, from a stream of their own - no draw of config() moves"""
    rng = np.random.default_rng([0x6B626F, int(seed), 3])
    n = len(lens)
    ex = {"legs": {name: bool(rng.random() < LEG2_P[name]) for name in LEGS2}}  # ("strands" below is which strands, not the leg)
    order = rng.permutation(n)
    minus = np.zeros(n, dtype=bool)
    minus[order[:(n + 1) // 2]] = True  # half of the sequences, whichever the batch's size
    ex["minus"] = tuple(bool(x) for x in minus)
    ex["strands"] = int(rng.choice([1, 2, 3, 3, 3, 3]))
    ex["strand_format"] = bool(rng.random() < 0.5)
    ex["strand_gap"] = int(rng.choice([0, 0, 3, 50]))
    ex["find_dev_gap"] = int(rng.choice([0, 0, 5, 2**32 - 1]))
    ex["find_dev_cap"] = float(rng.random())  # the second run's capacity, as a part of the oracle's count
    forms = {name: bool(rng.random() < p) for name, p in zip(SUMMARY_FORMS, (0.6, 0.5, 0.8, 0.6))}
    ex["summary_max_len_known"] = bool(rng.random() < 0.5)  # kbo_summary_dev / _words_dev: max_seq_len = the longest, or 0
    ns = n + len(short_seqs)  # (a threshold per sequence of the device legs' batch, with_shorts)
    choice = rng.integers(0, N_THR_CANDIDATES, ns)
    choice[:2] = (0, 1)[:ns]  # 2 and 3: two thresholds in every batch of two sequences or more, whatever t is
    ex["thr_choice"] = tuple(int(x) for x in choice)
    ex["rle_capacity_mode"] = str(rng.choice(["full", "third", "zero"]))
    ex["rle_gap"] = int(rng.choice([0, 3, 50, 2**32 - 1]))
    # map_reads_kernel's NP = 18 summary forms need reads over a depth table of order 16: the few configurations that have both run them
    if knobs["depth_table"] == 16 and max(lens) <= 160 and k >= 16:
        ex["legs"]["summary"] = forms["device"] = True
    ex["summary_forms"] = forms
    return ex


def thresholds_of(cfg, t, n_seqs):
    """the threshold of every sequence of the device legs' batch: cfg.extra["thr_choice"] into {2, 3, t - 1, t, t + 1, k - 1, k}
    clipped to [2, k], t the oracle's threshold -> int32[n_seqs]"""
    cand = np.clip(np.array([2, 3, t - 1, t, t + 1, cfg.k - 1, cfg.k], dtype=np.int64), 2, cfg.k)
    assert len(cand) == N_THR_CANDIDATES and len(cfg.extra["thr_choice"]) == n_seqs
    return cand[np.asarray(cfg.extra["thr_choice"], dtype=np.int64)].astype(np.int32)


def config(seed):
    """everything one iteration draws, from `seed` alone"""
    rng = np.random.default_rng([0x6B626F, int(seed)])
    cls = K_CLASSES[int(rng.integers(0, len(K_CLASSES)))]
    k = int(rng.choice(cls, p=[0.1, 0.15, 0.3, 0.45])) if cls is K_CLASSES[0] else int(rng.choice(cls))  # (k = 1, 2: little but refusals)
    G = int(rng.choice(GENOMES, p=[0.45, 0.45, 0.1]))  # (the oracle builds every index: its cost grows with k x G)
    if k <= 2:
        G = GENOMES[0]  # (over a large genome every k-mer of k <= 2 is there: the threshold is <= 1 and everything refuses)
    genome_seed = int(rng.integers(1, 1 << 30))
    repeats = bool(rng.random() < 0.3)
    several = bool(rng.random() < 0.35)
    n_contigs = int(rng.integers(2, 9)) if several else 1
    short_contigs = int(rng.integers(1, 4)) if several else 0
    rc = bool(rng.random() < 0.2)
    knobs = _knobs(rng)
    shape = str(rng.choice(["uniform", "ragged", "long", "mixed", "reads", "reads", "reads_uniform", "reads_boundary", "reads_boundary", "ragged_boundary",
                            "long_boundary", "long_boundary"]))
    lens = _lens(rng, k, shape, G)
    refuse_len = int(rng.integers(0, 3)) if rng.random() < 0.12 else -1
    refuse_at = int(rng.integers(0, len(lens) + 1))
    sub = float(rng.choice([0.0, 0.01, 0.05, 0.3], p=[0.15, 0.45, 0.3, 0.1]))
    indel = bool(rng.random() < 0.4)
    n_bytes = bool(rng.random() < 0.3)
    p_err = float(rng.choice([1e-7, 1e-7, 1e-7, 1e-3, 0.1]))
    gap_len = int(rng.choice([0, 0, 3, 50]))
    packed_gap_len = int(rng.choice([0, 2, 50]))
    legs = {name: bool(rng.random() < LEG_P[name]) for name in LEGS}
    call_emit = int(rng.choice([0, 1, 1, 2]))
    call_pick = tuple(int(x) for x in rng.integers(0, len(lens), 6))
    map_opts = (bool(rng.random() < 0.7), bool(rng.random() < 0.5), bool(rng.random() < 0.5))
    opts_lens = tuple(int(x) for x in rng.integers(max(2 * k + 64, 300), max(2 * k + 65, 4000), int(rng.integers(6, 30))))
    if legs["shards"] and n_contigs == 1:  # leg k: a sharded index is built from several contigs
        n_contigs, short_contigs = int(rng.integers(2, 9)), int(rng.integers(1, 4))
    n_short = int(rng.integers(1, 5)) if rng.random() < 0.5 else 0
    short_seqs = tuple(sorted((int(rng.integers(0, len(lens) + 1)), int(rng.integers(0, 3))) for _ in range(n_short)))
    extra = _extra(seed, k, knobs, lens, short_seqs)
    return Config(seed=int(seed), k=k, G=G, genome_seed=genome_seed, repeats=repeats, n_contigs=n_contigs, short_contigs=short_contigs,
                  add_revcomp=rc, knobs=knobs, shape=shape, lens=lens, short_seqs=short_seqs, refuse_len=refuse_len, refuse_at=refuse_at, sub_rate=sub, indel=indel, n_bytes=n_bytes,
                  max_error_prob=p_err, gap_len=gap_len, packed_gap_len=packed_gap_len, legs=legs, call_emit=call_emit,
                  call_pick=call_pick, map_opts=map_opts, opts_lens=opts_lens, dev_format=bool(rng.random() < 0.5),
                  dev_zero_sizing=bool(rng.random() < 0.3), tail_stream=bool(rng.random() < 0.5),
                  stream_pipelines=int(rng.integers(1, 3)), stream_parts=int(rng.integers(3, 7)), shards=int(rng.choice([2, 3])), extra=extra)


def _genome(cfg, rng):
    g = ACGT[rng.integers(0, 4, cfg.G)]
    if cfg.repeats:  # repeats and a non-ACGT byte in the index
        g = np.concatenate([g, np.tile(g[:int(rng.integers(20, 500))], int(rng.integers(2, 20))), [ord("N")], g[::-1][:1000]]).astype(np.uint8)
    return g


def _read(rng, g, n, sub, indel, n_bytes):
    s0 = int(rng.integers(0, len(g) - n))
    p = g[s0:s0 + n].copy()
    hit = rng.random(n) < sub
    p[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    if n_bytes and rng.random() < 0.05:
        p[rng.integers(0, n, max(1, n // 50))] = ord("N")
    if indel and n > 30 and rng.random() < 0.4:  # an insertion or a deletion of 1 - 3 bases, the length kept
        q = int(rng.integers(5, n - 5))
        w = int(rng.integers(1, 4))
        if rng.random() < 0.5:
            p = np.concatenate([p[:q], p[q + w:], ACGT[rng.integers(0, 4, w)]])
        else:
            p = np.concatenate([p[:q], ACGT[rng.integers(0, 4, w)], p[q:n - w]])
    return p


def make_inputs(cfg):
    """-> (contigs: list of bytes, concat uint8, offsets uint64[n + 1]) of the index and the main batch"""
    rng = np.random.default_rng([0x6B626F, int(cfg.seed), 1])
    g = _genome(cfg, rng)
    contigs = [g.tobytes()]
    if cfg.n_contigs > 1:
        cuts = np.sort(rng.choice(np.arange(1, len(g)), cfg.n_contigs - 1, replace=False))
        contigs = [x.tobytes() for x in np.split(g, cuts)]
        for _ in range(cfg.short_contigs):  # shorter than k: no k-mer of their own
            contigs.insert(int(rng.integers(0, len(contigs) + 1)), ACGT[rng.integers(0, 4, int(rng.integers(1, max(2, cfg.k))))].tobytes())
    pieces = [_read(rng, g, min(n, len(g) - 1), cfg.sub_rate, cfg.indel, cfg.n_bytes) for n in cfg.lens]
    lens = [len(p) for p in pieces]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return contigs, np.concatenate(pieces).astype(np.uint8), offsets


def with_shorts(cfg, concat, offsets, lengths=(0, 1, 2)):
    """the main batch with cfg.short_seqs (those of `lengths`) put in -> (concat, offsets, keep: bool per base, True for the bases of
    the main batch's own sequences, which are all of 3 bases or more)"""
    lens = np.diff(offsets.astype(np.int64))
    pieces, out_lens, at = [], [], 0
    for where, n in [x for x in cfg.short_seqs if x[1] in lengths] + [(len(lens), -1)]:
        a, b = int(offsets[at]), int(offsets[where])
        pieces.append(concat[a:b])
        out_lens += [int(x) for x in lens[at:where]]
        at = where
        if n >= 0:
            pieces.append(ACGT[(np.arange(n) + where) % 4])
            out_lens.append(n)
    out_lens = np.asarray(out_lens, dtype=np.int64)
    return (np.concatenate(pieces).astype(np.uint8), np.concatenate([[0], np.cumsum(out_lens)]).astype(np.uint64),
            np.repeat(out_lens >= 3, out_lens))


def with_refused(cfg, concat, offsets):
    """the main batch with the sequence of cfg.refuse_len bases put in at cfg.refuse_at"""
    lens = np.diff(offsets.astype(np.int64))
    a = int(offsets[cfg.refuse_at])
    concat2 = np.concatenate([concat[:a], concat[:cfg.refuse_len], concat[a:]]).astype(np.uint8)
    lens2 = np.concatenate([lens[:cfg.refuse_at], [cfg.refuse_len], lens[cfg.refuse_at:]])
    return concat2, np.concatenate([[0], np.cumsum(lens2)]).astype(np.uint64)


def revcomp(concat, offsets):
    """the reverse complement of every sequence in place of the sequence (kbo_hip.h "both strands"), in numpy"""
    off = np.asarray(offsets).astype(np.int64)
    lens = np.diff(off)
    src = np.repeat(off[:-1] + off[1:] - 1, lens) - np.arange(int(off[-1]), dtype=np.int64)  # base i of s <- base a + b - 1 - i
    return COMP[np.asarray(concat, dtype=np.uint8)[src]]


def make_strand_inputs(cfg, concat, offsets):
    """the main batch with the sequences of cfg.extra["minus"] reverse-complemented: the reads of the other strand, without which the
    '-' outputs over a forward-only index are all '-' and compare nothing -> concat"""
    minus = np.asarray(cfg.extra["minus"], dtype=bool)
    assert len(minus) == len(offsets) - 1
    per_base = np.repeat(minus, np.diff(np.asarray(offsets).astype(np.int64)))
    return np.where(per_base, revcomp(concat, offsets), concat).astype(np.uint8)


PACK_CODE = np.full(256, 4, dtype=np.uint8)
PACK_CODE[list(b"ACGT")] = (0, 1, 2, 3)


def pack_words(codes, offsets):
    """2-bit codes (one per base, 0 .. 3) -> the packed layout of kbo_hip.h: every sequence starts a word, 16 bases a word from the
    low bits up, the padding bits of a sequence's last word zero -> uint32 words"""
    off = np.asarray(offsets).astype(np.int64)
    lens = np.diff(off)
    wo = np.concatenate([[0], np.cumsum((lens + 15) // 16)])
    pos = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], lens)
    words = np.zeros(int(wo[-1]), dtype=np.uint64)
    np.add.at(words, np.repeat(wo[:-1], lens) + pos // 16, np.asarray(codes, dtype=np.uint64) << (2 * (pos % 16)).astype(np.uint64))
    return words.astype(np.uint32)


def pack_reads(concat, offsets):
    """bytes -> (words, exception positions uint64, exception bytes, mask of the bits that are specified: not those of a listed base)"""
    concat = np.asarray(concat, dtype=np.uint8)
    code = PACK_CODE[concat]
    pos = np.flatnonzero(code == 4).astype(np.uint64)
    mask = ~pack_words(np.where(code == 4, 3, 0), offsets)
    return pack_words(code & 3, offsets), pos, concat[pos.astype(np.int64)].copy(), mask


def genome_of(cfg):
    """the index text make_inputs() cut its contigs from"""
    return _genome(cfg, np.random.default_rng([0x6B626F, int(cfg.seed), 1]))


def make_opts_inputs(cfg, threshold=None):
    """-> (concat, offsets) of the batch of legs g / h (kbo_map_batch_opts / kbo_fill_gaps_batch, which take empty sequences): long
    sequences with a substituted block of 2 .. 40 bases between two matching flanks (a gap to fill), a few substitutions, sometimes an
    insertion or a deletion; then the lengths at which the entry points refuse one sequence: 0, 1, 2, 3, threshold - 1, threshold"""
    rng = np.random.default_rng([0x6B626F, int(cfg.seed), 2])
    g = genome_of(cfg)
    seqs = []
    for n in cfg.opts_lens:
        n = min(n, len(g) - 1)
        s0 = int(rng.integers(0, len(g) - n))
        p = g[s0:s0 + n].copy()
        for _ in range(int(rng.integers(1, 4))):
            w = int(rng.integers(2, 41))
            a = int(rng.integers(cfg.k + 8, max(cfg.k + 9, n - cfg.k - 8 - w)))
            if a + w < n:
                blk = p[a:a + w]
                p[a:a + w] = ACGT[(np.searchsorted(ACGT, np.where(np.isin(blk, ACGT), blk, ord("A"))) + rng.integers(1, 4, len(blk))) % 4]
        hit = rng.random(n) < min(cfg.sub_rate, 0.01)
        p[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        if cfg.indel and rng.random() < 0.4:
            q = int(rng.integers(5, n - 5))
            w = int(rng.integers(1, 20))
            p = np.concatenate([p[:q], p[q + w:]]) if rng.random() < 0.5 else np.concatenate([p[:q], ACGT[rng.integers(0, 4, w)], p[q:]])
        seqs.append(p.astype(np.uint8))
    t = int(threshold) if threshold else 12
    for n in (0, 1, 2, 3, max(3, t - 1), t, 2 * cfg.k + 2, 2 * cfg.k + 3):
        n = min(n, len(g) - 1)
        s0 = int(rng.integers(0, len(g) - n))
        seqs.insert(int(rng.integers(0, len(seqs) + 1)), g[s0:s0 + n].copy())
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return np.concatenate(seqs).astype(np.uint8), offsets


# The suite's fixed list (tests/test_gpu_random_configs.py runs exactly these; tools/stress.py draws seeds beyond it).
SEEDS = tuple(range(1, 241))
STRESS_FIRST_SEED = 100_000
