"""Python face of libraxtax_hip.so, mirroring the reference's interface for the hot path
(same names, argument meaning and error behaviour):

    Tree.new(lineages, sequences)            src/tree.rs:46-140   (host mirror)
    parse_reference_fasta_str(text) -> Tree  src/parser.rs:46-105
    parse_query_fasta_str(text, skip)        src/parser.rs:117-154
    raxtax(queries, tree, skip_exact_matches, raw_confidence, chunk_size, sender, tsv)
                                             src/raxtax.rs:14-97  (device path)
    Index(tree).classify(...)                the body of raxtax() without string formatting

Everything device-side goes through the C ABI (include/raxtax_hip.h).  No fallbacks.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import (RTX_MAX_DEPTH, RTX_RAW_CONFIDENCE, RTX_SKIP_EXACT_MATCHES, NodesView, ResultView, RtxError, check,
                   f32p, f64p, ptr, u8p, u16p, u32p, u64p)


def _flatten(seqs: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    flat = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
    for i, s in enumerate(seqs):
        flat[int(off[i]):int(off[i + 1])] = np.asarray(s, dtype=np.uint8)
    return flat, off


class Tree:
    """Host mirror of `Tree` (src/tree.rs:36-43)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        self._lib = _lib.load()

    def __del__(self):
        try:
            if self._h:
                self._lib.rtx_tree_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @classmethod
    def new(cls, lineages: Sequence[str], sequences: Sequence[np.ndarray]) -> "Tree":
        flat, off = _flatten(sequences)
        return cls.new_flat(lineages, flat, off)

    @classmethod
    def new_flat(cls, lineages: Sequence[str], seq_bytes: np.ndarray, seq_off: np.ndarray,
                 kmer_map: bool = True) -> "Tree":
        """kmer_map=False skips the host k-mer map; Index(tree) then builds the bitmaps on the GPU."""
        lib = _lib.load()
        enc = [l.encode() for l in lineages]
        loff = np.zeros(len(enc) + 1, dtype=np.uint64)
        if enc:
            loff[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
        lbytes = b"".join(enc)
        seq_bytes = np.ascontiguousarray(seq_bytes, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        h = C.c_void_p()
        check(lib.rtx_tree_build_ex(len(enc), lbytes, ptr(loff, u64p), ptr(seq_bytes, u8p), ptr(seq_off, u64p),
                                    0 if kmer_map else 1, C.byref(h)))
        return cls(h.value)

    def save_to_file(self, path: str) -> None:
        """Tree::save_to_file (tree.rs:147-153): the reference's bincode `.bin` database."""
        check(self._lib.rtx_tree_save_bin(self._h, str(path).encode()))

    @classmethod
    def load_from_file(cls, path: str) -> "Tree":
        """Tree::load_from_file (tree.rs:155-164)."""
        lib = _lib.load()
        h = C.c_void_p()
        check(lib.rtx_tree_load_bin(str(path).encode(), C.byref(h)))
        return cls(h.value)

    @property
    def num_tips(self) -> int:
        return self._lib.rtx_tree_num_tips(self._h)

    def lineage(self, i: int) -> str:
        return self._lib.rtx_tree_lineage(self._h, i).decode()

    @property
    def lineages(self) -> List[str]:
        return [self.lineage(i) for i in range(self.num_tips)]

    def original_index(self) -> np.ndarray:
        return np.array([self._lib.rtx_tree_original_index(self._h, i) for i in range(self.num_tips)], np.uint64)

    def csr(self) -> Tuple[np.ndarray, np.ndarray]:
        """Tree.k_mer_map as (offsets[65537], postings) -- views copied out of the handle."""
        po, pp = u64p(), u32p()
        check(self._lib.rtx_tree_kmer_csr(self._h, C.byref(po), C.byref(pp)))
        off = np.ctypeslib.as_array(po, shape=(65537,)).copy()
        tot = int(off[-1])
        post = np.ctypeslib.as_array(pp, shape=(tot,)).copy() if tot else np.zeros(0, np.uint32)
        return off, post

    def k_mer_map(self, kmer: int) -> np.ndarray:
        off, post = self.csr()
        return post[int(off[kmer]):int(off[kmer + 1])]

    def exact_matches(self, seq: np.ndarray) -> np.ndarray:
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        p = u32p()
        n = self._lib.rtx_tree_exact_matches(self._h, ptr(seq, u8p), len(seq), C.byref(p))
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)

    def exact_matches_batch(self, bases: np.ndarray, base_off: np.ndarray):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        n_q = len(base_off) - 1
        off = np.zeros(n_q + 1, dtype=np.uint64)
        ids = np.zeros(max(n_q, 16), dtype=np.uint32)
        tot = self._lib.rtx_tree_exact_matches_batch(self._h, n_q, ptr(bases, u8p), ptr(base_off, u64p), ptr(off, u64p),
                                                     ptr(ids, u32p), len(ids))
        if tot > len(ids):
            ids = np.zeros(tot, dtype=np.uint32)
            self._lib.rtx_tree_exact_matches_batch(self._h, n_q, ptr(bases, u8p), ptr(base_off, u64p), ptr(off, u64p),
                                                   ptr(ids, u32p), len(ids))
        return ids[:tot].copy(), off

    def nodes(self) -> dict:
        v = NodesView()
        check(self._lib.rtx_tree_nodes(self._h, C.byref(v)))
        n = v.n_nodes
        g = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy()
        return dict(begin=g(v.node_begin), end=g(v.node_end), first_child=g(v.node_first_child),
                    n_children=g(v.node_n_children), parent=g(v.node_parent), type=g(v.node_type))


def parse_reference_fasta_str(text: str) -> Tree:
    lib = _lib.load()
    b = text.encode()
    h = C.c_void_p()
    check(lib.rtx_tree_parse_reference_fasta(b, len(b), C.byref(h)))
    return Tree(h.value)


def parse_query_fasta_str(text: str, queries_to_skip: Sequence[str] = ()) -> List[Tuple[str, np.ndarray]]:
    lib = _lib.load()
    b = text.encode()
    skip = (C.c_char_p * max(len(queries_to_skip), 1))(*[s.encode() for s in queries_to_skip])
    h = C.c_void_p()
    check(lib.rtx_queries_parse_fasta(b, len(b), skip, len(queries_to_skip), C.byref(h)))
    try:
        n = lib.rtx_queries_len(h)
        pb, po = u8p(), u64p()
        check(lib.rtx_queries_data(h, C.byref(pb), C.byref(po)))
        off = np.ctypeslib.as_array(po, shape=(n + 1,)).copy()
        tot = int(off[-1])
        bases = np.ctypeslib.as_array(pb, shape=(tot,)).copy() if tot else np.zeros(0, np.uint8)
        return [(lib.rtx_queries_label(h, i).decode(), bases[int(off[i]):int(off[i + 1])].copy()) for i in range(n)]
    finally:
        lib.rtx_queries_destroy(h)


def parse_query_fastq_str(text: str, queries_to_skip: Sequence[str] = (), ascii_base: int = 33) -> List[Tuple[str, np.ndarray, np.ndarray]]:
    """rtx_queries_parse_fastq: (label, bases, quals) of every record of a FASTQ text in the four-line form; the bases encoded as
    parse_query_fasta_str encodes them, the quality bytes as they stand in the file (ASCII, ascii_base not taken off)."""
    lib = _lib.load()
    b = text.encode() if isinstance(text, str) else bytes(text)
    skip = (C.c_char_p * max(len(queries_to_skip), 1))(*[s.encode() for s in queries_to_skip])
    h = C.c_void_p()
    check(lib.rtx_queries_parse_fastq(b, len(b), skip, len(queries_to_skip), int(ascii_base), C.byref(h)))
    try:
        return _queries_records(lib, h)
    finally:
        lib.rtx_queries_destroy(h)


def _queries_records(lib, h):
    """The records of an rtx_queries handle: (label, bases) pairs, or (label, bases, quals) triples when it holds qualities."""
    n = lib.rtx_queries_len(h)
    pb, po, pq = u8p(), u64p(), u8p()
    check(lib.rtx_queries_data(h, C.byref(pb), C.byref(po)))
    check(lib.rtx_queries_quals(h, C.byref(pq)))
    off = np.ctypeslib.as_array(po, shape=(n + 1,)).copy()
    tot = int(off[-1])
    bases = np.ctypeslib.as_array(pb, shape=(tot,)).copy() if tot else np.zeros(0, np.uint8)
    if not pq:
        return [(lib.rtx_queries_label(h, i).decode(), bases[int(off[i]):int(off[i + 1])].copy()) for i in range(n)]
    quals = np.ctypeslib.as_array(pq, shape=(tot,)).copy() if tot else np.zeros(0, np.uint8)
    return [(lib.rtx_queries_label(h, i).decode(), bases[int(off[i]):int(off[i + 1])].copy(), quals[int(off[i]):int(off[i + 1])].copy()) for i in range(n)]


@dataclass
class EvaluationResult:
    """src/lineage.rs:8-14 (lineage given as index into tree.lineages)."""
    lineage: int
    node: int
    confidence_values: List[float]
    local_signal: float
    global_signal: float


class Result:
    """Arrays of one classified batch, copied out of the library-owned rtx_result_view and put into query
    order (the library stores the rows in processing order): rows of query q = row_off[q] .. row_off[q+1].
    strand (0 plus, 1 minus: Index(strand="both")) and peak (the largest hit count over the references for the classified orientation)
    per query, when the view came from a download (rtx_batch_strands), else None.  nearest (the lowest reference id whose hit count is the
    peak, NO_REF where the peak is 0) and nearest_ties (references with that count) per query under Index(nearest=True), else None.
    nearest_dist (the semi-global edit distance of the query, as classified, to that reference: semiglobal_distance; NO_DIST where there is
    none) and query_len (bases) per query under Index(identity=True), else None."""

    def __init__(self, view: ResultView, strand: Optional[np.ndarray] = None, peak: Optional[np.ndarray] = None,
                 nearest: Optional[np.ndarray] = None, nearest_ties: Optional[np.ndarray] = None,
                 nearest_dist: Optional[np.ndarray] = None, query_len: Optional[np.ndarray] = None):
        nq, nr = view.n_queries, view.n_rows
        self.strand, self.peak = strand, peak
        self.nearest, self.nearest_ties = nearest, nearest_ties
        self.nearest_dist, self.query_len = nearest_dist, query_len
        arr = lambda p, n: (np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0))
        self.n_queries = nq
        self.t = arr(view.t, nq)
        self.status = arr(view.status, nq)
        self.global_signal = arr(view.global_signal, nq)
        begin = arr(view.row_begin, nq).astype(np.int64)
        count = arr(view.row_count, nq).astype(np.int64)
        self.row_off = np.zeros(nq + 1, dtype=np.uint64)
        self.row_off[1:] = np.cumsum(count)
        # source row of every canonical row
        src = (np.repeat(begin - self.row_off[:-1].astype(np.int64), count) + np.arange(int(count.sum()))) if nq else np.zeros(0, np.int64)
        assert len(src) <= nr   # (under both strands the row arrays also hold the rows of the orientations that lost)
        self.row_lineage = arr(view.row_lineage, nr)[src]
        self.row_node = arr(view.row_node, nr)[src]
        self.row_depth = arr(view.row_depth, nr)[src]
        stride = int(view.row_conf_stride) or RTX_MAX_DEPTH     # ABI 5: the deepest lineage of the tree (0 in a hand-made view: RTX_MAX_DEPTH)
        self.row_conf = (np.ctypeslib.as_array(view.row_conf, shape=(nr, stride))[src] if nr
                         else np.zeros((0, stride)))
        self.row_local_signal = arr(view.row_local_signal, nr)[src]
        # the confidences as integer hundredths, [rows][stride] (what the taxon profile counts; a hand-made view has none: rounded from row_conf)
        self.row_conf_hundredths = (np.ctypeslib.as_array(view.row_conf_hundredths, shape=(nr, stride))[src].copy() if nr and view.row_conf_hundredths
                                    else np.rint(self.row_conf * 100.0).astype(np.uint8))

    def rows(self, q: int) -> List[EvaluationResult]:
        out = []
        for r in range(int(self.row_off[q]), int(self.row_off[q + 1])):
            d = int(self.row_depth[r])
            out.append(EvaluationResult(int(self.row_lineage[r]), int(self.row_node[r]),
                                        [float(x) for x in self.row_conf[r, :d]],
                                        float(self.row_local_signal[r]), float(self.global_signal[q])))
        return out


@dataclass
class Profile:
    """The taxon profile of a handle (rtx_index_profile_read), or a sum of several (profile_merge): per node of Tree.nodes() the queries under it
    (clade), assigned to it (direct) and the sum of their confidences in hundredths (conf_sum); totals = queries, classified, unclassified,
    unclassifiable.  cutoff in hundredths, flags = RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE as the profile was begun."""
    cutoff: int
    flags: int
    clade: np.ndarray
    direct: np.ndarray
    conf_sum: np.ndarray
    totals: np.ndarray

    def _view(self) -> "_lib.ProfileView":
        v = _lib.ProfileView()
        v.n_nodes, v.cutoff_hundredths, v.flags = len(self.clade), self.cutoff, self.flags
        v.clade, v.direct, v.conf_sum = ptr(self.clade, u64p), ptr(self.direct, u64p), ptr(self.conf_sum, u64p)
        for i in range(4):
            v.totals[i] = int(self.totals[i])
        return v


def profile_merge(profiles: Sequence[Profile]) -> Profile:
    """rtx_profile_merge: the sum of the profiles of several handles (one per GPU); they must agree on the nodes, the cutoff and the flags."""
    if not profiles:
        raise ValueError("profile_merge: no profiles")
    views = [p._view() for p in profiles]
    arr = (C.POINTER(_lib.ProfileView) * len(views))(*[C.pointer(v) for v in views])
    n = len(profiles[0].clade)
    clade, direct, conf = (np.zeros(n, np.uint64) for _ in range(3))
    totals = np.zeros(4, np.uint64)
    check(_lib.load().rtx_profile_merge(arr, len(views), ptr(clade, u64p), ptr(direct, u64p), ptr(conf, u64p), ptr(totals, u64p)))
    return Profile(profiles[0].cutoff, profiles[0].flags, clade, direct, conf, totals)


def profile_text(tree: Tree, profile: Profile) -> str:
    """rtx_profile_format: the report of a profile over `tree` (what raxtax-hip --profile writes to PREFIX/raxtax.profile)."""
    lib = _lib.load()
    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (profile.clade, profile.direct, profile.conf_sum, profile.totals)]
    args = [tree._h] + [ptr(x, u64p) for x in a] + [int(profile.cutoff)]
    n = check(lib.rtx_profile_format(*args, None, 0))
    buf = C.create_string_buffer(max(n, 1))
    check(lib.rtx_profile_format(*args, buf, n))
    return buf.raw[:n].decode()


@dataclass
class SampleProfile:
    """The per-sample counters beside a profile (rtx_index_profile_read_samples), or a sum of several (sample_profile_merge): direct[s][n] the
    queries of sample s assigned to node n of Tree.nodes(), totals[s] = queries, classified, unclassified, unclassifiable of sample s."""
    cutoff: int
    flags: int
    direct: np.ndarray
    totals: np.ndarray

    def _view(self) -> "_lib.SampleProfileView":
        self.direct = np.ascontiguousarray(self.direct, dtype=np.uint64)
        self.totals = np.ascontiguousarray(self.totals, dtype=np.uint64)
        v = _lib.SampleProfileView()
        v.n_samples, v.n_nodes = self.direct.shape
        v.cutoff_hundredths, v.flags = self.cutoff, self.flags
        v.direct, v.totals = ptr(self.direct, u64p), ptr(self.totals, u64p)
        return v


def sample_profile_merge(profiles: Sequence[SampleProfile]) -> SampleProfile:
    """rtx_sample_profile_merge: the sum of the per-sample counters of several handles (one per GPU); they must agree on the nodes, the samples,
    the cutoff and the flags."""
    if not profiles:
        raise ValueError("sample_profile_merge: no profiles")
    views = [p._view() for p in profiles]
    arr = (C.POINTER(_lib.SampleProfileView) * len(views))(*[C.pointer(v) for v in views])
    direct = np.zeros(profiles[0].direct.shape, np.uint64)
    totals = np.zeros((direct.shape[0], 4), np.uint64)
    check(_lib.load().rtx_sample_profile_merge(arr, len(views), ptr(direct if direct.size else np.zeros(1, np.uint64), u64p), ptr(totals, u64p)))
    return SampleProfile(profiles[0].cutoff, profiles[0].flags, direct, totals)


def sample_table_text(tree: Tree, names: Sequence[str], profile: SampleProfile) -> str:
    """rtx_sample_table_format: the taxon x sample table of per-sample clade counts over `tree` (what raxtax-hip --tags --profile writes to
    PREFIX/raxtax.samples); names: one per sample."""
    lib = _lib.load()
    direct = np.ascontiguousarray(profile.direct, dtype=np.uint64)
    totals = np.ascontiguousarray(profile.totals, dtype=np.uint64)
    if len(names) != direct.shape[0] or totals.shape != (direct.shape[0], 4):
        raise ValueError(f"sample_table_text: {len(names)} names, counters of shape {direct.shape} and {totals.shape}")
    cn = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    args = [tree._h, len(names), cn, ptr(direct if direct.size else np.zeros(1, np.uint64), u64p), ptr(totals, u64p), int(profile.cutoff)]
    n = check(lib.rtx_sample_table_format(*args, None, 0))
    buf = C.create_string_buffer(max(n, 1))
    check(lib.rtx_sample_table_format(*args, buf, n))
    return buf.raw[:n].decode()


DEFAULT_SEGMENT_CLASSES = 1   # RTX_DEFAULT_SEGMENT_CLASSES of the library (rtx_api_index.hip: g_seg_classes)


class Index:
    """Device-resident index + batch workspace of one GPU (rtx_index)."""

    identity_on = False  # Index(identity=True): downloads also fetch rtx_batch_identity
    nearest_on = False   # Index(nearest=True): downloads also fetch rtx_batch_nearest (the staged subclasses never set the option)

    def __init__(self, tree: Tree, device: int = 0, sub_batch: int = 0, prob_mode: int = 0,
                 stage_timing: bool = False, cluster: Optional[bool] = None, segment_classes=None,
                 packed_counts: Optional[bool] = None,
                 tile_skip: Optional[bool] = None, hit_pair=None, locator: Optional[bool] = None, tile_prune: Optional[bool] = None,
                 debug_taps: bool = False, device_exact: Optional[bool] = None, fine_bounds: Optional[bool] = None,
                 records: Optional[int] = None, overlap: Optional[bool] = None, two_level: Optional[int] = None,
                 prune_self_sample: Optional[bool] = None, device_text: bool = False, strand: str = "plus",
                 nearest: bool = False, derep: bool = False, identity: bool = False, primers=None, quality=None, chimera=None, tags=None, contaminants=None, tally=None):
        self._lib = _lib.load()
        self.tree = tree
        self._tally = None
        if segment_classes is None:
            segment_classes = DEFAULT_SEGMENT_CLASSES
        check(self._lib.rtx_set_default_option(1, int(segment_classes)))   # creation-time default of the library
        h = C.c_void_p()
        check(self._lib.rtx_index_create_from_tree(device, tree._h, C.byref(h)))
        self._h = h
        self.n_refs = self._lib.rtx_index_num_refs(self._h)
        if sub_batch:
            check(self._lib.rtx_index_set_batch(self._h, sub_batch))
        if prob_mode:
            check(self._lib.rtx_index_set_option(self._h, 2, prob_mode))
        if stage_timing:
            check(self._lib.rtx_index_set_option(self._h, 6, 1))
        if cluster is not None:
            check(self._lib.rtx_index_set_option(self._h, 7, int(cluster)))
        if packed_counts is not None:
            check(self._lib.rtx_index_set_option(self._h, 8, int(packed_counts)))
        if tile_skip is not None:
            check(self._lib.rtx_index_set_option(self._h, 10, int(tile_skip)))
        if hit_pair is not None:
            check(self._lib.rtx_index_set_option(self._h, 11, int(hit_pair)))
        if locator is not None:
            check(self._lib.rtx_index_set_option(self._h, 12, int(locator)))
        if tile_prune is not None:
            check(self._lib.rtx_index_set_option(self._h, 13, int(tile_prune)))
            # NOTE: an explicit tile_prune=True also sets RTX_OPT_PRUNE_SELF_SAMPLE = 0 -- it asks for the pruned path whatever the
            # handle's self-sample said (A/B tests); the C API keeps the two options independent.  Pass prune_self_sample=True to keep the verdict.
            if tile_prune and prune_self_sample is None:
                check(self._lib.rtx_index_set_option(self._h, 22, 0))
        if debug_taps:
            check(self._lib.rtx_index_set_option(self._h, 14, 1))
        if device_exact is not None:
            check(self._lib.rtx_index_set_option(self._h, 15, int(device_exact)))
        if device_text:   # RTX_OPT_DEVICE_TEXT: raxtax() takes the lines of its chunks from the device (rtx_text.hip)
            check(self._lib.rtx_index_set_option(self._h, 24, 1))
        if fine_bounds is not None:
            check(self._lib.rtx_index_set_option(self._h, 17, int(fine_bounds)))
        if records is not None:   # RTX_OPT_RECORDS: pruned queries with at most this many live tiles write records instead of counts (0: off)
            check(self._lib.rtx_index_set_option(self._h, 18, int(records)))
        if overlap is not None:   # RTX_OPT_OVERLAP: back half of a sub-batch on a second stream beside the front half of the next
            check(self._lib.rtx_index_set_option(self._h, 19, int(overlap)))
        if two_level is not None:  # RTX_OPT_TWO_LEVEL_BOUNDS: 0 = the bounds pass over blocks of 64 throughout (values above 1: the refine rule, packed)
            check(self._lib.rtx_index_set_option(self._h, 21, int(two_level)))
        if prune_self_sample is not None:  # RTX_OPT_PRUNE_SELF_SAMPLE: False = RTX_OPT_TILE_PRUNE alone decides (tests of the pruned path on real barcodes)
            check(self._lib.rtx_index_set_option(self._h, 22, int(prune_self_sample)))
        if strand not in ("plus", "both"):
            raise ValueError(f"strand must be 'plus' or 'both', not {strand!r}")
        self.strand = strand
        if strand == "both":   # RTX_OPT_STRAND: every query is classified in both orientations, the one with the larger peak is reported
            check(self._lib.rtx_index_set_option(self._h, 25, 1))
        self.nearest_on = bool(nearest) or bool(identity)
        if self.nearest_on:   # RTX_OPT_NEAREST: every run also names the reference that holds each query's peak
            check(self._lib.rtx_index_set_option(self._h, 26, 1))
        self.identity_on = bool(identity)
        if identity:   # RTX_OPT_IDENTITY: ... and aligns the query to it (rtx_identity.hip); implies nearest
            check(self._lib.rtx_index_set_option(self._h, 28, 1))
        if derep:   # RTX_OPT_DEREP: raxtax() classifies each distinct read of a chunk once (rtx_derep.hip); classify() ignores it
            check(self._lib.rtx_index_set_option(self._h, _lib.RTX_OPT_DEREP, 1))
        if primers:   # rtx_index_set_primers: raxtax() trims every read with them first (rtx_trim.hip); classify() ignores them
            self.set_primers(primers)
        if tags:   # rtx_index_set_tags: raxtax() assigns every read to a sample and cuts its tags first (rtx_demux.hip); classify() ignores them
            self.set_tags(*tags)
        if quality is not None:   # rtx_index_set_quality: raxtax() filters every read by its quality string (rtx_qual.hip); classify() ignores it
            self.set_quality(quality)
        if chimera is not None:   # rtx_index_set_chimera: raxtax() checks every read against the references first (rtx_chimera.hip); classify() ignores it
            self.set_chimera(ChimeraParams() if chimera is True else chimera)
        if contaminants is not None:   # rtx_index_set_screen: raxtax() screens every read against the set first (rtx_screen.hip); classify() ignores it
            self.set_screen(*(contaminants if isinstance(contaminants, tuple) else (contaminants,)))
        if tally is not None:   # rtx_index_set_tally: raxtax() tallies the reads it classifies into the object (rtx_tally.hip); classify() ignores it
            self.set_tally(tally)
        self._view = ResultView()
        self._keep = None

    def set_tally(self, tally) -> None:
        """rtx_index_set_tally: the Tally raxtax() counts the classified reads into (on the handle's device); None switches it off."""
        check(self._lib.rtx_index_set_tally(self._h, tally._h if tally is not None else None))
        self._tally = tally   # (the object is the caller's: kept alive as long as the handle names it)

    @property
    def tally(self):
        """The Tally the handle holds, or None (rtx_index_tally)."""
        return self._tally if self._lib.rtx_index_tally(self._h) else None

    def set_screen(self, sset, params=None) -> None:
        """rtx_index_set_screen: the ScreenSet and ScreenParams raxtax() screens every read with; None switches the stage off.  The handle
        keeps what it needs of the set."""
        if sset is None:
            check(self._lib.rtx_index_set_screen(self._h, None, None))
        else:
            check(self._lib.rtx_index_set_screen(self._h, sset._h, C.byref((params or ScreenParams())._c())))

    @property
    def screen(self):
        """(ScreenParams, fingerprint of the keys and the parameters) the handle holds, or None (rtx_index_screen)."""
        c, on, fp = _lib.ScreenParams(), C.c_int(), C.c_uint64()
        check(self._lib.rtx_index_screen(self._h, C.byref(c), C.byref(on), C.byref(fp)))
        return (ScreenParams(c.min_hits, c.min_pct), int(fp.value)) if on.value else None

    def set_quality(self, params) -> None:
        """rtx_index_set_quality: the QualParams raxtax() filters every read with (its queries then come with quality strings); None, or
        parameters that are entirely off, switch the stage off."""
        check(self._lib.rtx_index_set_quality(self._h, C.byref(params._c()) if params is not None else None))

    @property
    def quality(self):
        """The QualParams the handle holds, or None (rtx_index_quality)."""
        c, on = _lib.QualParams(), C.c_int()
        check(self._lib.rtx_index_quality(self._h, C.byref(c), C.byref(on)))
        return QualParams._of(c) if on.value else None

    def set_chimera(self, params) -> None:
        """rtx_index_set_chimera: the ChimeraParams raxtax() checks every read with; None switches the stage off."""
        check(self._lib.rtx_index_set_chimera(self._h, C.byref(params._c()) if params is not None else None))

    @property
    def chimera(self):
        """The ChimeraParams the handle holds, or None (rtx_index_chimera)."""
        c, on = _lib.ChimeraParams(), C.c_int()
        check(self._lib.rtx_index_chimera(self._h, C.byref(c), C.byref(on)))
        return ChimeraParams(c.segments, c.mindelta) if on.value else None

    def set_tags(self, tags, pairs=(), params=None) -> None:
        """rtx_index_set_tags: the tags (DemuxTag or (codes, end)), pairs ((tag5, tag3, sample), None: no tag at that end) and DemuxParams (see
        sample_sheet) raxtax() demultiplexes every read with; an empty tag list switches the stage off."""
        arr, n_tags, parr, n_pairs, cp, _keep = _demux_args(tags, pairs, params)
        check(self._lib.rtx_index_set_tags(self._h, arr, n_tags, parr, n_pairs, C.byref(cp)))

    @property
    def tags(self) -> int:
        """How many tags the handle holds (rtx_index_tags)."""
        n = C.c_uint32()
        check(self._lib.rtx_index_tags(self._h, C.byref(n)))
        return int(n.value)

    def set_primers(self, patterns) -> None:
        """rtx_index_set_primers: the patterns (TrimPrimer, or (codes, end, max_errors[, window]) tuples; see primer_patterns) raxtax()
        trims every read with; an empty list switches the stage off."""
        arr, _keep = _trim_patterns(patterns)
        check(self._lib.rtx_index_set_primers(self._h, arr, len(_keep)))

    @property
    def primers(self) -> int:
        """How many patterns the handle holds (rtx_index_primers)."""
        n = C.c_uint32()
        check(self._lib.rtx_index_primers(self._h, C.byref(n)))
        return int(n.value)

    @property
    def prune_verdict(self):
        """(tile pruning is on for this handle, share of (query, tile) combinations its self-sample kept live or -1): rtx_index_prune_verdict."""
        on, frac = C.c_int(), C.c_double()
        check(self._lib.rtx_index_prune_verdict(self._h, C.byref(on), C.byref(frac)))
        return bool(on.value), float(frac.value)

    @property
    def run_ahead_stats(self):
        """(batches enqueued ahead of the end of the batch before them, run-aheads abandoned) under RTX_OPT_RUN_AHEAD: rtx_index_run_ahead_stats."""
        a, b = C.c_uint64(), C.c_uint64()
        check(self._lib.rtx_index_run_ahead_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def __del__(self):
        try:
            if self._h:
                self._lib.rtx_index_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        return self._lib.rtx_index_device_bytes(self._h)

    @property
    def workspace_bytes(self) -> int:
        """HBM of everything else the handle holds as of the last upload (tables, scratch sets, inputs, result arrays)."""
        return self._lib.rtx_index_workspace_bytes(self._h)

    def workspace_parts(self) -> dict:
        out = np.zeros(9, dtype=np.uint64)
        check(self._lib.rtx_index_workspace_parts(self._h, ptr(out, u64p)))
        names = ("prob_tables", "counts", "record_segments", "prefix_sums", "tile_masks_and_slot_lists", "other_scratch", "inputs_and_order", "results")
        d = {k: int(v) for k, v in zip(names, out[:8])}
        d["scratch_sets"] = int(out[8])
        return d

    # ---- staged interface -------------------------------------------------------------
    def upload(self, bases: np.ndarray, base_off: np.ndarray, exact_ids: Optional[np.ndarray] = None,
               exact_off: Optional[np.ndarray] = None):
        self.prefetch(bases, base_off, exact_ids, exact_off)
        self.activate()

    def prefetch(self, bases: np.ndarray, base_off: np.ndarray, exact_ids: Optional[np.ndarray] = None,
                 exact_off: Optional[np.ndarray] = None):
        """Stages a batch beside the current one (rtx_batch_prefetch): packed, pinned, asynchronous H2D; activate() makes it current."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        n_q = len(base_off) - 1
        if exact_off is not None:
            exact_off = np.ascontiguousarray(exact_off, dtype=np.uint64)
            exact_ids = np.ascontiguousarray(exact_ids if exact_ids is not None and len(exact_ids) else
                                             np.zeros(1, np.uint32), dtype=np.uint32)
            check(self._lib.rtx_batch_prefetch(self._h, n_q, ptr(bases, u8p), ptr(base_off, u64p), ptr(exact_ids, u32p),
                                               ptr(exact_off, u64p)))
        else:
            check(self._lib.rtx_batch_prefetch(self._h, n_q, ptr(bases, u8p), ptr(base_off, u64p), None, None))

    def prefetch_weights(self, weights: np.ndarray):
        """One weight per query of the batch the NEXT prefetch() / upload() / classify() stages: the reads it stands for in the open profile
        (rtx_batch_prefetch_weights).  A count that does not match that batch is dropped."""
        w = np.ascontiguousarray(weights, dtype=np.uint32)
        check(self._lib.rtx_batch_prefetch_weights(self._h, len(w), ptr(w if len(w) else np.zeros(1, np.uint32), u32p)))

    def prefetch_samples(self, samples: np.ndarray):
        """One sample per query of the batch the NEXT prefetch() / upload() / classify() stages, for the per-sample counters of the open profile
        (rtx_batch_prefetch_samples); DEMUX_NONE: the query counts in no sample.  A count that does not match that batch is dropped."""
        s = np.ascontiguousarray(samples, dtype=np.uint32)
        check(self._lib.rtx_batch_prefetch_samples(self._h, len(s), ptr(s if len(s) else np.zeros(1, np.uint32), u32p)))

    def activate(self):
        check(self._lib.rtx_batch_activate(self._h))

    def run(self, flags: int = 0):
        check(self._lib.rtx_batch_run(self._h, flags))

    def sync(self):
        check(self._lib.rtx_batch_sync(self._h))

    def download(self, copy: bool = True):
        check(self._lib.rtx_batch_download(self._h, C.byref(self._view)))
        if not copy:
            return self._view
        return Result(self._view, *self.strands(), *(self.nearest() if self.nearest_on else (None, None)),
                      *(self.identity() if self.identity_on else (None, None)))

    def identity(self):
        """(dist, qlen) of every query of the last download: rtx_batch_identity (Index(identity=True))."""
        pd, pl = u32p(), u32p()
        check(self._lib.rtx_batch_identity(self._h, C.byref(pd), C.byref(pl)))
        n = self._view.n_queries
        if not n:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(pd, shape=(n,)).copy(), np.ctypeslib.as_array(pl, shape=(n,)).copy()

    def identity_time(self):
        """(milliseconds, launches) of the kernels behind identity() in the last run (stage_timing=True): rtx_batch_identity_time."""
        ms, n = C.c_float(), C.c_uint32()
        check(self._lib.rtx_batch_identity_time(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def nearest(self):
        """(nearest, ties) of every query of the last download: rtx_batch_nearest (Index(nearest=True))."""
        pn, pt = u32p(), u32p()
        check(self._lib.rtx_batch_nearest(self._h, C.byref(pn), C.byref(pt)))
        n = self._view.n_queries
        if not n:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(pn, shape=(n,)).copy(), np.ctypeslib.as_array(pt, shape=(n,)).copy()

    def nearest_time(self):
        """(milliseconds, launches) of the kernel behind nearest() in the last run (stage_timing=True): rtx_batch_nearest_time."""
        ms, n = C.c_float(), C.c_uint32()
        check(self._lib.rtx_batch_nearest_time(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    # ---- taxon profile (rtx_profile.hip) ----------------------------------------------------
    def profile_begin(self, cutoff: float = 0.8, skip_exact_matches: bool = False, raw_confidence: bool = False, n_samples: Optional[int] = None):
        """Opens the taxon profile of the handle: every batch downloaded from now on is added once (rtx_index_profile_begin).  cutoff: the
        confidence a level needs to count, in (0, 1]; either flag switches the single-exact-match override off, as in the `.out` text.
        n_samples: also count per sample (rtx_index_profile_begin_samples; prefetch_samples() names the sample of every query,
        profile_read_samples() reads the counters)."""
        flags = (RTX_SKIP_EXACT_MATCHES if skip_exact_matches else 0) | (RTX_RAW_CONFIDENCE if raw_confidence else 0)
        if n_samples is None:
            check(self._lib.rtx_index_profile_begin(self._h, int(round(cutoff * 100)), flags))
        else:
            check(self._lib.rtx_index_profile_begin_samples(self._h, int(round(cutoff * 100)), flags, int(n_samples)))

    def profile_read_samples(self) -> "SampleProfile":
        v = _lib.SampleProfileView()
        check(self._lib.rtx_index_profile_read_samples(self._h, C.byref(v)))
        nn, ns = int(v.n_nodes), int(v.n_samples)
        direct = np.ctypeslib.as_array(v.direct, shape=(ns, nn)).copy() if nn else np.zeros((ns, 0), np.uint64)
        return SampleProfile(int(v.cutoff_hundredths), int(v.flags), direct, np.ctypeslib.as_array(v.totals, shape=(ns, 4)).copy())

    def profile_read(self) -> Profile:
        v = _lib.ProfileView()
        check(self._lib.rtx_index_profile_read(self._h, C.byref(v)))
        n = v.n_nodes
        g = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        return Profile(int(v.cutoff_hundredths), int(v.flags), g(v.clade), g(v.direct), g(v.conf_sum), np.array(list(v.totals), dtype=np.uint64))

    def profile_reset(self):
        check(self._lib.rtx_index_profile_reset(self._h))

    def profile_end(self):
        check(self._lib.rtx_index_profile_end(self._h))

    def profile_time(self):
        """(milliseconds, launches) of the profile kernel since profile_begin / profile_reset (stage_timing=True): rtx_index_profile_time."""
        ms, n = C.c_float(), C.c_uint32()
        check(self._lib.rtx_index_profile_time(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def strands(self):
        """(strand, peak) of every query of the last download: rtx_batch_strands."""
        ps, pk = u8p(), u32p()
        check(self._lib.rtx_batch_strands(self._h, C.byref(ps), C.byref(pk)))
        n = self._view.n_queries
        if not n:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(ps, shape=(n,)).copy(), np.ctypeslib.as_array(pk, shape=(n,)).copy()

    def stage_times(self):
        ms = (C.c_float * len(_lib.STAGES))()
        n = (C.c_uint32 * len(_lib.STAGES))()
        check(self._lib.rtx_batch_stage_times(self._h, ms, n))
        return {s: (float(ms[i]), int(n[i])) for i, s in enumerate(_lib.STAGES)}

    def work(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.rtx_batch_work(self._h, C.byref(a), C.byref(b), C.byref(c)))
        live, bounds = C.c_uint64(), C.c_uint64()
        check(self._lib.rtx_batch_work_split(self._h, C.byref(live), C.byref(bounds)))
        return dict(sum_hits=a.value, sum_query_bytes=b.value, bitmap_bytes_read=c.value, live_bytes=live.value, bounds_bytes=bounds.value)

    def prob_work(self):
        """Grid points D_q (n_q + 1) of prob.rs:43-90 summed over the queries of the last run."""
        a, b = C.c_uint64(), C.c_uint64()
        check(self._lib.rtx_batch_prob_work(self._h, C.byref(a), C.byref(b)))
        return dict(grid_points=a.value, distinct_counts=b.value)

    # ---- one call -----------------------------------------------------------------------
    def exact_matches(self, bases: np.ndarray, base_off: np.ndarray):
        """Tree.sequences.get() for every query (raxtax.rs:42) on the HOST -> (ids, offsets)."""
        return self.tree.exact_matches_batch(bases, base_off)

    @property
    def has_exact_lookup(self) -> bool:
        """The handle looks exact matches up itself when a batch comes without ids (rtx_exact.hip)."""
        return bool(self._lib.rtx_index_has_exact_lookup(self._h))

    def device_exact_matches(self):
        """Tree.sequences.get() for every query of the last download as the DEVICE found it -> (ids, offsets)."""
        po, pi = u64p(), u32p()
        check(self._lib.rtx_batch_exact_matches(self._h, C.byref(po), C.byref(pi)))
        n = self._view.n_queries
        off = np.ctypeslib.as_array(po, shape=(n + 1,)).copy()
        tot = int(off[-1])
        ids = np.ctypeslib.as_array(pi, shape=(tot,)).copy() if tot else np.zeros(0, np.uint32)
        return ids, off

    def classify(self, bases: np.ndarray, base_off: np.ndarray, exact_ids=None, exact_off=None,
                 skip_exact_matches: bool = False) -> Result:
        """exact_off = None: the exact matches are looked up on the device (has_exact_lookup), else the batch has none."""
        self.upload(bases, base_off, exact_ids, exact_off)
        self.run(RTX_SKIP_EXACT_MATCHES if skip_exact_matches else 0)
        return self.download()

    def classify_text(self, bases: np.ndarray, base_off: np.ndarray, labels: Sequence, exact_ids=None, exact_off=None,
                      skip_exact_matches: bool = False, raw_confidence: bool = False, tsv: bool = False):
        """classify() with the result text formatted on the device (rtx_text.hip) -> (out_texts, tsv_texts or None), one str per query in
        input order: the lines rtx_format_query prints for it ('\\n'-joined; '' for a query with status != 0).  The view of the download
        stays available (format_query, rows)."""
        flags = (RTX_SKIP_EXACT_MATCHES if skip_exact_matches else 0) | (_lib.RTX_RAW_CONFIDENCE if raw_confidence else 0) | (_lib.RTX_TEXT_TSV if tsv else 0)
        check(self._lib.rtx_index_text_setup(self._h, self.tree._h, flags))
        n_q = len(base_off) - 1
        if len(labels) != n_q:
            raise ValueError(f"{len(labels)} labels for {n_q} queries")
        labs = (C.c_char_p * max(n_q, 1))(*[l.encode() if isinstance(l, str) else bytes(l) for l in labels])
        check(self._lib.rtx_batch_prefetch_labels(self._h, n_q, labs))
        self.prefetch(bases, base_off, exact_ids, exact_off)
        self.activate()
        self.run(RTX_SKIP_EXACT_MATCHES if skip_exact_matches else 0)
        self.download(copy=False)
        return self.last_text()

    def last_text(self):
        """The device text of the last download (rtx_batch_text) -> (out_texts, tsv_texts or None)."""
        tv = _lib.TextView()
        check(self._lib.rtx_batch_text(self._h, C.byref(tv)))
        n = tv.n_queries

        def split(base, off_p):
            off = np.ctypeslib.as_array(off_p, shape=(n + 1,)).astype(np.int64)
            raw = C.string_at(base, int(off[-1])) if off[-1] else b""
            return [raw[off[q]:off[q + 1] - 1].decode() for q in range(n)]

        return split(tv.out, tv.out_off), (split(tv.tsv, tv.tsv_off) if tv.tsv else None)

    # ---- parity taps ----------------------------------------------------------------------
    def debug_kmers(self, q: int) -> np.ndarray:
        out = np.zeros(65536, dtype=np.uint16)
        t = C.c_uint32()
        check(self._lib.rtx_debug_kmers(self._h, q, ptr(out, u16p), C.byref(t)))
        return out[:t.value].copy()

    def debug_hit_counts(self, q: int) -> np.ndarray:
        out = np.zeros(self.n_refs, dtype=np.uint16)
        check(self._lib.rtx_debug_hit_counts(self._h, q, ptr(out, u16p)))
        return out

    def debug_prob_table(self, q: int, t: int):
        out = np.zeros(t + 1, dtype=np.float64)
        z = C.c_double()
        check(self._lib.rtx_debug_prob_table(self._h, q, ptr(out, f64p), C.byref(z)))
        return out, z.value

    def debug_pruned_prob_table(self, q: int, t: int):
        """table / Z of query q as the pruned run computed it, Z and the query's threshold (before any other tap)."""
        out = np.zeros(t + 1, dtype=np.float64)
        z = C.c_double()
        thr = C.c_uint32()
        check(self._lib.rtx_debug_pruned_prob_table(self._h, q, ptr(out, f64p), C.byref(z), C.byref(thr)))
        return out, z.value, int(thr.value)

    def debug_run_counts(self, q: int, t: int) -> dict:
        """Query q of the last sub-batch exactly as the (pruned) run left it -- no recount; before any other tap.  counts (0xFFFF in
        tiles hit_count did not visit), tile_live, hist (bin 0 = never-counted references + counted ones without a hit), threshold, i1."""
        counts = np.zeros(self.n_refs, dtype=np.uint16)
        live = np.zeros((self.n_refs + 8191) // 8192, dtype=np.uint8)
        hist = np.zeros(t + 1, dtype=np.uint32)
        thr, i1 = C.c_uint32(), C.c_uint32()
        check(self._lib.rtx_debug_run_counts(self._h, q, ptr(counts, u16p), ptr(live, u8p), ptr(hist, u32p), C.byref(thr), C.byref(i1)))
        nseg = C.c_uint32()
        check(self._lib.rtx_debug_run_mode(self._h, q, C.byref(nseg)))
        # record_segments > 0: the query took the records path (RTX_OPT_RECORDS) -- `counts` of its visited tiles hold the count of every
        # reference ABOVE the threshold and 0 for the others (it wrote records of those alone)
        return dict(counts=counts, tile_live=live.astype(bool), hist=hist, threshold=int(thr.value), i1=int(i1.value), record_segments=int(nseg.value))

    def debug_tile_bounds(self, q: int) -> np.ndarray:
        """The largest bound of every tile as the bounds pass left it for query q of the last sub-batch."""
        out = np.zeros((self.n_refs + 8191) // 8192, dtype=np.uint16)
        check(self._lib.rtx_debug_tile_bounds(self._h, q, ptr(out, u16p)))
        return out

    def debug_prune_detail(self, q: int) -> dict:
        """prune_kernel's view of query q (Index(debug_taps=True)): best block, its exact counts, M, threshold, i* + 1."""
        out = np.zeros(72, dtype=np.uint32)
        check(self._lib.rtx_debug_prune_detail(self._h, q, ptr(out, u32p)))
        return dict(block=int(out[0]), M=int(out[1]), threshold=int(out[2]), i1=int(out[3]), largest_bound=int(out[4]), t=int(out[5]),
                    block_counts=out[8:72].copy())

    def debug_probs(self, q: int) -> np.ndarray:
        out = np.zeros(self.n_refs, dtype=np.float64)
        check(self._lib.rtx_debug_probs(self._h, q, ptr(out, f64p)))
        return out

    def sub_batch_size(self) -> int:
        """Queries per sub-batch (kernel launch) of the uploaded batch."""
        b, n = C.c_uint32(), C.c_uint32()
        check(self._lib.rtx_batch_sub_batch(self._h, C.byref(b), C.byref(n)))
        return int(b.value)

    def last_sub_batch(self):
        """(first position, queries) of the last sub-batch of the uploaded batch in the processing order: what the taps can read."""
        first, n = C.c_uint64(), C.c_uint32()
        check(self._lib.rtx_batch_last_sub_batch(self._h, C.byref(first), C.byref(n)))
        return int(first.value), int(n.value)

    def batch_classes(self) -> list:
        """Length classes of the uploaded batch: dicts of queries, longest query, sub-batch size, planes and what the class runs through."""
        n = C.c_uint32()
        out = np.zeros(20, dtype=np.uint64)
        check(self._lib.rtx_batch_classes(self._h, C.byref(n), ptr(out, u64p)))
        res = []
        for c in range(int(n.value)):
            f = int(out[4 * c + 3])
            res.append(dict(queries=int(out[4 * c]), longest=int(out[4 * c + 1]), sub_batch=int(out[4 * c + 2]), planes=f & 0xFF, tables=bool(f >> 8 & 1),
                            pair=bool(f >> 9 & 1), prune=bool(f >> 10 & 1), records=bool(f >> 11 & 1), global_memory_forms=bool(f >> 12 & 1)))
        return res

    def debug_order(self, n_queries: int) -> np.ndarray:
        """Processing order of the last run: perm[position] = query."""
        out = np.zeros(n_queries, dtype=np.uint32)
        check(self._lib.rtx_debug_order(self._h, ptr(out, u32p)))
        return out

    def debug_prune_stats(self) -> dict:
        """Tile pruning of the last run: live tiles per pair, mean lower bound of the best hit, mean threshold, mean largest tile bound."""
        out = np.zeros(16, dtype=np.uint64)
        check(self._lib.rtx_debug_prune_stats(self._h, ptr(out, u64p)))
        pairs, nq = max(int(out[1]), 1), max(int(out[5]), 1)
        counted = int(out[12]) if int(out[11]) or int(out[12]) else int(out[0])   # after the fine bounds pass, if it ran
        return {"live_tiles_per_pair": counted / pairs, "live_tiles_per_pair_first_stage": int(out[0]) / pairs,
                "fine_blocks_per_pair": int(out[11]) / pairs, "fine_cleared_per_query": int(out[10]) / nq, "pairs": int(out[1]), "mean_best_hit_lower_bound": int(out[2]) / nq,
                "mean_threshold": int(out[3]) / nq, "mean_largest_tile_bound": int(out[4]) / nq, "bound_violations": int(out[6]), "live_tiles_per_query": int(out[7]) / nq,
                "tiles_above_threshold_per_query": int(out[8]) / max(int(out[9]), 1), "queries_with_threshold": int(out[9]),
                "record_queries": int(out[14]), "records_per_record_query": int(out[13]) / max(int(out[14]), 1), "record_slow_path_queries": int(out[15])}

    def debug_evaluate(self, probs, mode: int = 0) -> Result:
        """Lineage::new(label, tree, probs).evaluate() on the device (lineage.rs:61-112).  mode 0: the walk as a kernel of its own; 1: fused into
        taxon_prefix, as a run has it; 2: with tile maxima as well, so that tiles without a probability are skipped (rtx_debug_evaluate_mode).
        last_evaluate_table_in_lds tells whether the launch read the probability table from LDS."""
        probs = np.ascontiguousarray(probs, dtype=np.float64)
        assert len(probs) == self.n_refs
        in_lds = C.c_uint32()
        check(self._lib.rtx_debug_evaluate_mode(self._h, ptr(probs, f64p), mode, C.byref(self._view), C.byref(in_lds)))
        self.last_evaluate_table_in_lds = bool(in_lds.value)
        return Result(self._view)

    def debug_prob_hist(self, ts, hists, n_refs: int, kernel: int, thr=None, i1=None) -> dict:
        """The probability kernels on given histograms (rtx_debug_prob_hist): ts [n_q], hists [n_q, hstride] (hstride > max t; n_refs is the N of the
        global signal's 1 / N and enters nothing else).  kernel 0: the lookup in the memoised tables (thr / i1: the thresholds of a pruned run), 1: the recurrence in LDS,
        2: the recurrence in global memory.  table_z is NaN at the counts a histogram does not hold."""
        ts = np.ascontiguousarray(ts, dtype=np.uint32)
        hists = np.ascontiguousarray(hists, dtype=np.uint32)
        assert hists.ndim == 2 and hists.shape[0] == len(ts)
        n_q, hstride = hists.shape
        tz = np.zeros((n_q, hstride), dtype=np.float64)
        z = np.zeros(n_q, dtype=np.float64)
        gs = np.zeros(n_q, dtype=np.float64)
        status = np.zeros(n_q, dtype=np.uint8)
        ndist = np.zeros(n_q, dtype=np.uint32)
        if thr is not None:
            thr = np.ascontiguousarray(thr, dtype=np.uint16)
            i1 = np.ascontiguousarray(i1, dtype=np.uint16)
            assert len(thr) == n_q and len(i1) == n_q
        check(self._lib.rtx_debug_prob_hist(self._h, n_q, ptr(ts, u32p), ptr(hists, u32p), hstride, int(n_refs), int(kernel),
                                            ptr(thr, u16p) if thr is not None else None, ptr(i1, u16p) if thr is not None else None,
                                            ptr(tz, f64p), ptr(z, f64p), ptr(gs, f64p), ptr(status, u8p), ptr(ndist, u32p)))
        return {"table_z": tz, "z": z, "gs": gs, "status": status, "ndist": ndist}

    def format_query(self, q: int, label: str, seq: np.ndarray, exact_ids: np.ndarray, flags: int = 0,
                     tsv: bool = False):
        """Lines of query q of the last download (after override raxtax.rs:73-84)."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ex = np.ascontiguousarray(exact_ids if len(exact_ids) else np.zeros(1, np.uint32), dtype=np.uint32)
        cap = 1 << 20
        out = C.create_string_buffer(cap)
        tbuf = C.create_string_buffer(cap) if tsv else None
        tlen = C.c_int64()
        n = self._lib.rtx_format_query(self.tree._h, C.byref(self._view), q, label.encode(), ptr(seq, u8p), len(seq),
                                       ptr(ex, u32p), len(exact_ids), flags, out, cap, tbuf, cap, C.byref(tlen))
        check(n)
        return out.raw[:n].decode(), (tbuf.raw[:tlen.value].decode() if tsv else None)


_SENDER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p)
_INFO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32)
_HIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
_ALIGN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
NO_REF = 0xFFFFFFFF   # RTX_NO_REF
NO_DIST = 0xFFFFFFFF  # RTX_NO_DIST
_TRIM = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
TRIM_5P, TRIM_3P, TRIM_NO_PATTERN = _lib.RTX_TRIM_5P, _lib.RTX_TRIM_3P, _lib.RTX_TRIM_NO_PATTERN
IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "W": 9, "S": 6, "M": 3, "K": 12, "R": 5, "Y": 10, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}


@dataclass
class TrimPrimer:
    """One pattern of the primer trimming (rtx_trim_pattern): its codes (1 .. 15, at most 64), the end it is looked for at (TRIM_5P / TRIM_3P; a
    3' pattern as it reads on the read, 5'->3'), the errors allowed (fewer than its codes) and the window (0: min(256, len + max_errors + 32))."""
    codes: np.ndarray
    end: int
    max_errors: int
    window: int = 0


def encode_iupac(text: str) -> np.ndarray:
    """The codes of an oligo given in IUPAC letters (either case); ValueError names a character that is none."""
    try:
        return np.array([IUPAC[ch] for ch in text.upper()], np.uint8)
    except KeyError as e:
        raise ValueError(f"primer {text!r}: {e.args[0]!r} is no IUPAC code") from None


def primer_patterns(pair: Tuple[str, str], error_percent: int = 10, window: int = 0, both_strands: bool = False) -> List[TrimPrimer]:
    """The pattern list of a (FWD, REV) pair of oligos as ordered, 5'->3' (what raxtax-hip --primers FWD:REV registers): FWD at the 5' end and
    revcomp(REV) at the 3' end; both_strands=True adds REV at 5' and revcomp(FWD) at 3' (reads given in either orientation).  Either oligo may be
    empty.  max_errors = len * error_percent // 100."""
    fwd, rev = (encode_iupac(x) for x in pair)
    out = []

    def add(codes, end):
        if len(codes):
            out.append(TrimPrimer(codes, end, len(codes) * int(error_percent) // 100, window))

    add(fwd, TRIM_5P)
    add(revcomp(rev) if len(rev) else rev, TRIM_3P)
    if both_strands:
        add(rev, TRIM_5P)
        add(revcomp(fwd) if len(fwd) else fwd, TRIM_3P)
    return out


def _trim_patterns(patterns):
    """(rtx_trim_pattern array, the arrays it points into) of TrimPrimer objects or (codes, end, max_errors[, window]) tuples."""
    ps = [p if isinstance(p, TrimPrimer) else TrimPrimer(*p) for p in patterns]
    keep = [np.ascontiguousarray(p.codes, dtype=np.uint8) for p in ps]
    arr = (_lib.TrimPattern * max(len(ps), 1))()
    for i, (p, k) in enumerate(zip(ps, keep)):
        arr[i].codes = ptr(k if len(k) else np.zeros(1, np.uint8), u8p)
        arr[i].len, arr[i].end, arr[i].max_errors, arr[i].window = len(k), int(p.end), int(p.max_errors), int(p.window)
    return arr, keep


def trim_hit(hit: int) -> Tuple[Optional[int], int, Optional[int], int]:
    """(pattern5 or None, errors5, pattern3 or None, errors3) of a hit word: pat5 | err5 << 8 | pat3 << 16 | err3 << 24."""
    hit = int(hit)
    p5, e5, p3, e3 = hit & 0xFF, (hit >> 8) & 0xFF, (hit >> 16) & 0xFF, (hit >> 24) & 0xFF
    return (None if p5 == TRIM_NO_PATTERN else p5), e5, (None if p3 == TRIM_NO_PATTERN else p3), e3


def primer_search(pattern: np.ndarray, read: np.ndarray, end: int = TRIM_5P, window: int = 0, max_errors: int = 0) -> Tuple[int, int]:
    """rtx_primer_search: (cut, errors) of one pattern in one read on the host, with the function the device kernel calls; (0, NO_DIST) when
    not found."""
    p = np.ascontiguousarray(pattern, dtype=np.uint8)
    x = np.ascontiguousarray(read, dtype=np.uint8)
    one = np.zeros(1, np.uint8)
    cut, err = C.c_uint32(), C.c_uint32()
    check(_lib.load().rtx_primer_search(ptr(p if len(p) else one, u8p), len(p), ptr(x if len(x) else one, u8p), len(x), int(end), int(window),
                                        int(max_errors), C.byref(cut), C.byref(err)))
    return int(cut.value), int(err.value)


def trim_apply(bases: np.ndarray, base_off: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """rtx_trim_apply: (bases, offsets) of the kept ranges [lo, hi) of the reads, back to back."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
    lo = np.ascontiguousarray(lo, dtype=np.uint32)
    hi = np.ascontiguousarray(hi, dtype=np.uint32)
    n = len(base_off) - 1
    if len(lo) != n or len(hi) != n:
        raise ValueError(f"{len(lo)} / {len(hi)} ranges for {n} reads")
    out = np.zeros(max(len(bases), 1), np.uint8)
    off = np.zeros(n + 1, np.uint64)
    z8, z32 = np.zeros(1, np.uint8), np.zeros(1, np.uint32)
    check(_lib.load().rtx_trim_apply(n, ptr(bases if len(bases) else z8, u8p), ptr(base_off, u64p), ptr(lo if n else z32, u32p),
                                     ptr(hi if n else z32, u32p), ptr(out, u8p), ptr(off, u64p)))
    return out[:int(off[-1])].copy(), off


class _Stage:
    """What the stage classes share: the library, the handle of their C object rtx_<_c>, its release through rtx_<_c>_destroy and its times."""

    _c = ""  # trim, demux, qual, screen, chimera, merge, derep

    def _open(self, *args):
        self._lib = _lib.load()
        self._h = None
        h = C.c_void_p()
        check(getattr(self._lib, f"rtx_{self._c}_create")(*args, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                getattr(self._lib, f"rtx_{self._c}_destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def _kernel_ms(self) -> float:
        ms = C.c_float()
        check(getattr(self._lib, f"rtx_{self._c}_kernel_time")(self._h, C.byref(ms)))
        return float(ms.value)

    def _stage_seconds(self) -> Tuple[float, float, float]:
        t = (C.c_double * 3)()
        check(getattr(self._lib, f"rtx_{self._c}_stage_times")(self._h, t))
        return float(t[0]), float(t[1]), float(t[2])


class Trim(_Stage):
    """The primer-trimming stage on one GPU (rtx_trim): an object of its own beside any Index, one stream, buffers that only grow."""

    _c = "trim"

    def __init__(self, device: int, patterns):
        arr, keep = _trim_patterns(patterns)
        self._open(device, arr, len(keep))

    def run(self, bases: np.ndarray, base_off: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(lo, hi, hit) per read (rtx_trim_run): the read keeps [lo, hi); hit as trim_hit() takes it apart."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        n = len(base_off) - 1
        lo, hi, hit = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        check(self._lib.rtx_trim_run(self._h, n, ptr(bases if len(bases) else np.zeros(1, np.uint8), u8p), ptr(base_off, u64p), ptr(lo, u32p),
                                     ptr(hi, u32p), ptr(hit, u32p)))
        return lo[:n], hi[:n], hit[:n]

    def kernel_ms(self) -> float:
        """Milliseconds of the kernel of the last run(), from HIP events (rtx_trim_kernel_time)."""
        return self._kernel_ms()


def raxtax_last_trim() -> Tuple[int, int, int, int, float]:
    """rtx_raxtax_last_trim: (queries, with a 5' primer, with a 3' primer, left empty, busy seconds of the stage) of the last raxtax() call of
    this process; all 0 when its handles had no primers set."""
    a, b, c, d, s = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    check(_lib.load().rtx_raxtax_last_trim(C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(s)))
    return int(a.value), int(b.value), int(c.value), int(d.value), float(s.value)


_DEMUX = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
DEMUX_NO_TAG, DEMUX_NONE = _lib.RTX_DEMUX_NO_TAG, _lib.RTX_DEMUX_NONE
DEMUX_OK, DEMUX_NO_TAG5, DEMUX_NO_TAG3, DEMUX_AMBIGUOUS, DEMUX_UNKNOWN_PAIR = range(5)


@dataclass
class DemuxTag:
    """One inline tag of the sample demultiplexing (rtx_demux_tag): its codes (1 .. 15, at most 32) and the end it stands at (TRIM_5P /
    TRIM_3P; a 3' tag as it reads on the read, 5'->3')."""
    codes: np.ndarray
    end: int


@dataclass
class DemuxParams:
    """rtx_demux_params: the substitutions a tag may carry (at most 8) and the bases that may stand in front of it (at most 15)."""
    max_mismatches: int = 0
    max_offset: int = 0


def _demux_args(tags, pairs, params):
    """(rtx_demux_tag array, n_tags, rtx_demux_pair array, n_pairs, rtx_demux_params, the arrays they point into) of DemuxTag objects or
    (codes, end) tuples, (tag5, tag3, sample) triples (None: no tag at that end) and a DemuxParams or (max_mismatches, max_offset)."""
    ts = [t if isinstance(t, DemuxTag) else DemuxTag(*t) for t in tags]
    keep = [np.ascontiguousarray(t.codes, dtype=np.uint8) for t in ts]
    arr = (_lib.DemuxTag * max(len(ts), 1))()
    for i, (t, k) in enumerate(zip(ts, keep)):
        arr[i].codes = ptr(k if len(k) else np.zeros(1, np.uint8), u8p)
        arr[i].len, arr[i].end = len(k), int(t.end)
    pairs = list(pairs)
    parr = (_lib.DemuxPair * max(len(pairs), 1))()
    for i, (a, b, s) in enumerate(pairs):
        parr[i].tag5 = DEMUX_NO_TAG if a is None else int(a)
        parr[i].tag3 = DEMUX_NO_TAG if b is None else int(b)
        parr[i].sample = int(s)
    p = params if isinstance(params, DemuxParams) else DemuxParams(*(params or ()))
    return arr, len(ts), parr, len(pairs), _lib.DemuxParams(int(p.max_mismatches), int(p.max_offset)), keep


def demux_hit(hit: int, info: int) -> Tuple[int, Optional[int], int, int, Optional[int], int, int]:
    """(verdict, tag5 or None, mismatches5, offset5, tag3 or None, mismatches3, offset3) of a read's hit and info words."""
    hit, info = int(hit), int(info)
    t5, t3 = hit & 0xFFFF, hit >> 16
    return (info & 0xFF, None if t5 == DEMUX_NO_TAG else t5, (info >> 8) & 0xFF, (info >> 24) & 0xF,
            None if t3 == DEMUX_NO_TAG else t3, (info >> 16) & 0xFF, (info >> 28) & 0xF)


def demux_verdict_names() -> Tuple[str, ...]:
    """The name of every verdict of the demultiplexing, by its code."""
    return _lib.RTX_DEMUX_NAMES


def demux_read(tags, pairs, params, read: np.ndarray) -> Tuple[int, int, int, int, int]:
    """rtx_demux_read: (sample, lo, hi, hit, info) of one read on the host, with the function the device kernel calls."""
    arr, n_tags, parr, n_pairs, cp, _keep = _demux_args(tags, pairs, params)
    x = np.ascontiguousarray(read, dtype=np.uint8)
    out = [C.c_uint32() for _ in range(5)]
    check(_lib.load().rtx_demux_read(C.byref(cp), arr, n_tags, parr, n_pairs, ptr(x if len(x) else np.zeros(1, np.uint8), u8p), len(x),
                                     *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


class Demux(_Stage):
    """The sample-demultiplexing stage on one GPU (rtx_demux): an object of its own beside any Index, one stream, buffers that only grow."""

    _c = "demux"

    def __init__(self, device: int, tags, pairs, params=None):
        arr, n_tags, parr, n_pairs, cp, _keep = _demux_args(tags, pairs, params)
        self._open(device, arr, n_tags, parr, n_pairs, C.byref(cp))

    def run(self, bases: np.ndarray, base_off: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(sample, lo, hi, hit, info) per read (rtx_demux_run): the read belongs to `sample` (DEMUX_NONE: to none) and keeps [lo, hi);
        hit and info as demux_hit() takes them apart."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        n = len(base_off) - 1
        out = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(5)]
        check(self._lib.rtx_demux_run(self._h, n, ptr(bases if len(bases) else np.zeros(1, np.uint8), u8p), ptr(base_off, u64p),
                                      *[ptr(o, u32p) for o in out]))
        return tuple(o[:n] for o in out)

    def kernel_ms(self) -> float:
        """Milliseconds of the kernel of the last run(), from HIP events (rtx_demux_kernel_time)."""
        return self._kernel_ms()


def raxtax_last_demux() -> Tuple[int, int, List[int], float]:
    """rtx_raxtax_last_demux: (queries, assigned to a sample, queries of every verdict by its code, busy seconds of the stage) of the last
    raxtax() call of this process; all 0 when its handles had no tags set."""
    q, a, s = C.c_uint64(), C.c_uint64(), C.c_double()
    reasons = (C.c_uint64 * 5)()
    check(_lib.load().rtx_raxtax_last_demux(C.byref(q), C.byref(a), reasons, C.byref(s)))
    return int(q.value), int(a.value), [int(r) for r in reasons], float(s.value)


def sample_sheet(text: str, both_orientations: bool = False) -> Tuple[List[DemuxTag], List[Tuple[Optional[int], Optional[int], int]], List[str]]:
    """(tags, pairs, names) of a sample sheet: tab-separated lines `sample<TAB>fwd_tag<TAB>rev_tag` in IUPAC letters, `#` starts a comment.
    rev_tag is written as on the oligo (the read ends with its reverse complement); empty or `-`: single-ended.  A sample may own several
    lines; samples are numbered by first appearance, a tag that several lines share is listed once.  both_orientations=True adds the flipped
    layout of every line for the same sample: rev_tag at 5' and the reverse complement of fwd_tag at 3'.  ValueError names a malformed line
    and a (fwd_tag, rev_tag) pair that two lines give."""
    tags: List[DemuxTag] = []
    place = {}
    pairs, names, seen = [], [], {}

    def tag(codes, end):
        key = (bytes(codes), end)
        if key not in place:
            place[key] = len(tags)
            tags.append(DemuxTag(np.array(codes, np.uint8), end))
        return place[key]

    def add(t5, t3, sample, line_no):
        if (t5, t3) in seen:
            raise ValueError(f"sample sheet line {line_no}: the tag pair is given twice (line {seen[(t5, t3)]})")
        seen[(t5, t3)] = line_no
        pairs.append((t5, t3, sample))

    for line_no, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].rstrip()
        if not line.strip():
            continue
        f = [x.strip() for x in line.split("\t")]
        if len(f) < 2 or len(f) > 3 or not f[0] or not f[1]:
            raise ValueError(f"sample sheet line {line_no}: expected sample<TAB>fwd_tag<TAB>rev_tag")
        fwd = encode_iupac(f[1])
        rev = encode_iupac(f[2]) if len(f) == 3 and f[2] not in ("", "-") else None
        if f[0] not in names:
            names.append(f[0])
        sample = names.index(f[0])
        add(tag(fwd, TRIM_5P), None if rev is None else tag(revcomp(rev), TRIM_3P), sample, line_no)
        if both_orientations:
            if rev is None:   # (a single-ended pair holds only while the list has no tag at the other end: the flipped line would add one)
                raise ValueError(f"sample sheet line {line_no}: both_orientations needs a rev_tag")
            add(tag(rev, TRIM_5P), tag(revcomp(fwd), TRIM_3P), sample, line_no)
    return tags, pairs, names


_QUAL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32)
QUAL_MAX_READ = _lib.RTX_QUAL_MAX_READ
QC_BAD_QUALITY, QC_SHORT_FOR_TRUNC_LEN, QC_TOO_SHORT, QC_TOO_LONG, QC_TOO_MANY_N, QC_MAX_EE, QC_MAX_EE_RATE = (1 << b for b in range(7))


@dataclass
class QualParams:
    """The quality filter's parameters (rtx_qual_params); every field but ascii_base (33 or 64) has a value that switches it off.
    trunc_len: a range shorter than this is discarded, otherwise it is cut to this length; trunc_qual: cut in front of the first base with
    Q <= this; trunc_ee: ... in front of the first base at which the running sum of error probabilities is above this; min_len / max_len:
    discard by the kept length; max_ns: ... if the kept bases hold more non-A/C/G/T bases; max_ee: ... if their expected errors are above
    this; max_ee_rate: ... above this times the kept length.  A threshold x is compared as floor(x * 2^40)."""
    ascii_base: int = 33
    trunc_len: int = 0
    trunc_qual: int = -1
    trunc_ee: float = -1.0
    min_len: int = 0
    max_len: int = 0
    max_ns: int = -1
    max_ee: float = -1.0
    max_ee_rate: float = -1.0

    def _c(self) -> "_lib.QualParams":
        return _lib.QualParams(int(self.ascii_base), int(self.trunc_len), int(self.trunc_qual), float(self.trunc_ee), int(self.min_len), int(self.max_len),
                               int(self.max_ns), float(self.max_ee), float(self.max_ee_rate))

    @staticmethod
    def _of(c) -> "QualParams":
        return QualParams(c.ascii_base, c.trunc_len, c.trunc_qual, c.trunc_ee, c.min_len, c.max_len, c.max_ns, c.max_ee, c.max_ee_rate)


def qual_error_table() -> List[int]:
    """rtx_qual_error_table: e[Q] = llround(10^(-Q/10) * 2^40) for Q = 0 .. 93, the integers the device sums."""
    t = np.zeros(_lib.RTX_QUAL_TABLE, np.uint64)
    check(_lib.load().rtx_qual_error_table(ptr(t, u64p)))
    return [int(x) for x in t]


def qual_verdict_names(v: int) -> List[str]:
    """The reasons of a verdict (RTX_QC_*), [] for a read that passes."""
    return [name for b, name in enumerate(_lib.RTX_QC_NAMES) if (int(v) >> b) & 1]


def qual_read(params: QualParams, bases: np.ndarray, quals: np.ndarray, lo: int = 0, hi: Optional[int] = None) -> Tuple[int, int, int]:
    """rtx_qual_read: (hi, ee, verdict) of ONE read on the host, with the functions the device kernel calls; [lo, hi) is the input range
    (the whole read by default), ee the expected errors of the kept bases times 2^40."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    if len(bases) != len(quals):
        raise ValueError(f"{len(quals)} quality bytes for {len(bases)} bases")
    one = np.zeros(1, np.uint8)
    h, e, v = C.c_uint32(), C.c_uint64(), C.c_uint32()
    check(_lib.load().rtx_qual_read(C.byref(params._c()), ptr(bases if len(bases) else one, u8p), ptr(quals if len(quals) else one, u8p), len(bases),
                                    int(lo), len(bases) if hi is None else int(hi), C.byref(h), C.byref(e), C.byref(v)))
    return int(h.value), int(e.value), int(v.value)


class Qual(_Stage):
    """The quality-filter stage on one GPU (rtx_qual): an object of its own beside any Index, one stream, buffers that only grow."""

    _c = "qual"

    def __init__(self, device: int, params: QualParams):
        self._open(device, C.byref(params._c()))

    def run(self, bases: np.ndarray, quals: np.ndarray, base_off: np.ndarray, lo=None, hi=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(hi, ee, verdict) per read (rtx_qual_run): the read keeps [lo, hi) -- lo as given, 0 by default -- with ee expected errors
        times 2^40; verdict 0: it passes (qual_verdict_names)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        if len(bases) != len(quals):
            raise ValueError(f"{len(quals)} quality bytes for {len(bases)} bases")
        if (lo is None) != (hi is None):
            raise ValueError("Qual.run: give both lo and hi, or neither")
        n = len(base_off) - 1
        one = np.zeros(1, np.uint8)
        hi_out, verdict = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
        ee = np.zeros(max(n, 1), dtype=np.uint64)
        if lo is not None:
            lo = np.ascontiguousarray(lo, dtype=np.uint32)
            hi = np.ascontiguousarray(hi, dtype=np.uint32)
            if len(lo) != n or len(hi) != n:
                raise ValueError(f"{len(lo)} / {len(hi)} ranges for {n} reads")
            if n == 0:
                lo = hi = np.zeros(1, np.uint32)
        check(self._lib.rtx_qual_run(self._h, n, ptr(bases if len(bases) else one, u8p), ptr(quals if len(quals) else one, u8p), ptr(base_off, u64p),
                                     ptr(lo, u32p) if lo is not None else None, ptr(hi, u32p) if hi is not None else None, ptr(hi_out, u32p),
                                     ptr(ee, u64p), ptr(verdict, u32p)))
        return hi_out[:n], ee[:n], verdict[:n]

    def kernel_ms(self) -> float:
        """Milliseconds of the kernel of the last run(), from HIP events (rtx_qual_kernel_time)."""
        return self._kernel_ms()

    def stage_seconds(self) -> Tuple[float, float, float]:
        """(host staging, copies and waiting around the kernel, the whole call) of the last run(), in seconds (rtx_qual_stage_times)."""
        return self._stage_seconds()


def raxtax_last_qual() -> Tuple[int, int, int, List[int], float]:
    """rtx_raxtax_last_qual: (queries, passed, passed and cut short, how often each reason applied -- in the order of qual_verdict_names --
    busy seconds of the stage) of the last raxtax() call of this process; all 0 when its handles had no quality filter set."""
    a, b, c, s = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    r = (C.c_uint64 * 7)()
    check(_lib.load().rtx_raxtax_last_qual(C.byref(a), C.byref(b), C.byref(c), r, C.byref(s)))
    return int(a.value), int(b.value), int(c.value), [int(x) for x in r], float(s.value)


_SCREEN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
SCREEN_K, SCREEN_NONE, SCREEN_MAX_READ, SCREEN_MAX_BASES, SCREEN_CONTAMINANT = (_lib.RTX_SCREEN_K, _lib.RTX_SCREEN_NONE, _lib.RTX_SCREEN_MAX_READ, _lib.RTX_SCREEN_MAX_BASES,
                                                                                 _lib.RTX_SCREEN_CONTAMINANT)


@dataclass
class ScreenParams:
    """The contaminant screen's parameters (rtx_screen_params): a read is a contaminant iff at least min_hits of its valid 16-base windows
    are in the set and they are at least min_pct percent of its valid windows."""
    min_hits: int = 2
    min_pct: int = 50

    def _c(self) -> "_lib.ScreenParams":
        return _lib.ScreenParams(int(self.min_hits), int(self.min_pct))


class ScreenSet:
    """The canonical 16-mers of contaminant sequences as the table the device probes (rtx_screen_set): built on the host from FASTA text
    (read with the query parser: the labels need no lineage), from (label, bases) records or from plain code arrays.  Immutable."""

    def __init__(self, records_or_fasta_text):
        self._lib = _lib.load()
        self._h = None
        if isinstance(records_or_fasta_text, (str, bytes)):
            records_or_fasta_text = parse_query_fasta_str(records_or_fasta_text)
        recs = [r if isinstance(r, tuple) else ("", r) for r in records_or_fasta_text]
        self.labels = [r[0] for r in recs]
        flat, off = _flatten([np.ascontiguousarray(r[1], dtype=np.uint8) for r in recs])
        self._build(flat, off)

    @classmethod
    def from_arrays(cls, bases: np.ndarray, base_off: np.ndarray, labels=None) -> "ScreenSet":
        """The set of the sequences bases[base_off[i] : base_off[i + 1]] (rtx_screen_set_build as it stands)."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h = None
        self.labels = list(labels) if labels is not None else [""] * (len(base_off) - 1)
        self._build(np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(base_off, dtype=np.uint64))
        return self

    def _build(self, flat, off):
        h = C.c_void_p()
        check(self._lib.rtx_screen_set_build(len(off) - 1, ptr(flat if len(flat) else np.zeros(1, np.uint8), u8p), ptr(off, u64p), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                self._lib.rtx_screen_set_free(self._h)
                self._h = None
        except Exception:
            pass

    def info(self) -> dict:
        """rtx_screen_set_info: the number of keys, the slots of the table, the longest displacement of a stored key, the keys stored below
        their home slot (their chain wrapped) and the fingerprint of the keys."""
        v = [C.c_uint64() for _ in range(5)]
        check(self._lib.rtx_screen_set_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("keys", "slots", "max_displacement", "wrapped", "fingerprint"), (int(x.value) for x in v)))

    def table(self) -> Tuple[np.ndarray, int]:
        """rtx_screen_set_table: (the slots as [m, 2] uint32 -- key, src -- and log2 m)."""
        p, lg = u32p(), C.c_uint32()
        check(self._lib.rtx_screen_set_table(self._h, C.byref(p), C.byref(lg)))
        return np.ctypeslib.as_array(p, shape=(1 << lg.value, 2)).copy(), int(lg.value)


def screen_read(sset: ScreenSet, params: ScreenParams, bases: np.ndarray, lo: int = 0, hi: Optional[int] = None) -> Tuple[int, int, int, int, int]:
    """rtx_screen_read: (windows, hits, first, source, verdict) of ONE read on the host, with the functions the device kernel calls; [lo, hi)
    is the input range (the whole read by default), first counts from lo."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    one = np.zeros(1, np.uint8)
    v = [C.c_uint32() for _ in range(5)]
    check(_lib.load().rtx_screen_read(sset._h, C.byref(params._c()), ptr(bases if len(bases) else one, u8p), len(bases), int(lo),
                                      len(bases) if hi is None else int(hi), *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


class Screen(_Stage):
    """The contaminant-screen stage on one GPU (rtx_screen): an object of its own beside any Index, one stream, buffers that only grow,
    the table of the set uploaded once."""

    _c = "screen"

    def __init__(self, device: int, sset: ScreenSet, params: Optional[ScreenParams] = None):
        self._open(device, sset._h, C.byref((params or ScreenParams())._c()))

    def run(self, bases: np.ndarray, base_off: np.ndarray, lo=None, hi=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(windows, hits, first, source, verdict) per read (rtx_screen_run) over [lo, hi) -- the whole read by default; first counts from lo."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        if (lo is None) != (hi is None):
            raise ValueError("Screen.run: give both lo and hi, or neither")
        n = len(base_off) - 1
        out = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(5)]
        if lo is not None:
            lo = np.ascontiguousarray(lo, dtype=np.uint32)
            hi = np.ascontiguousarray(hi, dtype=np.uint32)
            if len(lo) != n or len(hi) != n:
                raise ValueError(f"{len(lo)} / {len(hi)} ranges for {n} reads")
            if n == 0:
                lo = hi = np.zeros(1, np.uint32)
        check(self._lib.rtx_screen_run(self._h, n, ptr(bases if len(bases) else np.zeros(1, np.uint8), u8p), ptr(base_off, u64p),
                                       ptr(lo, u32p) if lo is not None else None, ptr(hi, u32p) if hi is not None else None, *[ptr(a, u32p) for a in out]))
        return tuple(a[:n] for a in out)

    def kernel_ms(self) -> float:
        """Milliseconds of the kernel of the last run(), from HIP events (rtx_screen_kernel_time)."""
        return self._kernel_ms()

    def stage_seconds(self) -> Tuple[float, float, float]:
        """(host staging, copies and waiting around the kernel, the whole call) of the last run(), in seconds (rtx_screen_stage_times)."""
        return self._stage_seconds()


def raxtax_last_screen() -> Tuple[int, int, int, float]:
    """rtx_raxtax_last_screen: (queries, those whose range was not already empty, the contaminants among them, busy seconds of the stage)
    of the last raxtax() call of this process; all 0 when its handles had no screen set."""
    a, b, c, s = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    check(_lib.load().rtx_raxtax_last_screen(C.byref(a), C.byref(b), C.byref(c), C.byref(s)))
    return int(a.value), int(b.value), int(c.value), float(s.value)


_CHIM = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.POINTER(_lib.ChimeraRec))
CHIMERA_MAX_QUERY = _lib.RTX_CHIMERA_MAX_QUERY
CHIM_OK, CHIM_NO_KMER, CHIM_TOO_LONG = _lib.RTX_CHIM_OK, _lib.RTX_CHIM_NO_KMER, _lib.RTX_CHIM_TOO_LONG
CHIMERA_DTYPE = np.dtype([(f, np.uint32) for f in _lib.RTX_CHIM_FIELDS])   # rtx_chimera_rec


@dataclass
class ChimeraParams:
    """The chimera check's parameters (rtx_chimera_params): a read is cut into `segments` parts (2 .. 32) of its 8-mer windows, and flagged
    when the best pair of references over a left and a right part explains `mindelta` windows more than the best single reference."""
    segments: int = _lib.RTX_CHIMERA_DEFAULT_SEGMENTS
    mindelta: int = _lib.RTX_CHIMERA_DEFAULT_MINDELTA

    def _c(self) -> "_lib.ChimeraParams":
        return _lib.ChimeraParams(int(self.segments), int(self.mindelta))


def chimera_read(params: ChimeraParams, read: np.ndarray, ref_bases: np.ndarray, ref_off: np.ndarray) -> np.void:
    """rtx_chimera_read: the record (a CHIMERA_DTYPE scalar) of ONE read on the host, computed from the reference sequences."""
    read = np.ascontiguousarray(read, dtype=np.uint8)
    ref_bases = np.ascontiguousarray(ref_bases, dtype=np.uint8)
    ref_off = np.ascontiguousarray(ref_off, dtype=np.uint64)
    one = np.zeros(1, np.uint8)
    rec = np.zeros(1, CHIMERA_DTYPE)
    check(_lib.load().rtx_chimera_read(C.byref(params._c()), ptr(read if len(read) else one, u8p), len(read), ptr(ref_bases if len(ref_bases) else one, u8p),
                                       ptr(ref_off, u64p), len(ref_off) - 1, rec.ctypes.data_as(C.c_void_p)))
    return rec[0]


class Chimera(_Stage):
    """The chimera check in front of one Index (rtx_chimera): one stream and buffers of its own; it borrows the handle's bitmap, so it keeps
    the Index alive."""

    _c = "chimera"

    def __init__(self, index: "Index", params: Optional[ChimeraParams] = None):
        self._index = index
        self._open(index._h, C.byref((params or ChimeraParams())._c()))

    def run(self, bases: np.ndarray, base_off: np.ndarray) -> np.ndarray:
        """One record per read (rtx_chimera_run), as a structured array of CHIMERA_DTYPE."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        n = len(base_off) - 1
        out = np.zeros(max(n, 1), CHIMERA_DTYPE)
        check(self._lib.rtx_chimera_run(self._h, n, ptr(bases if len(bases) else np.zeros(1, np.uint8), u8p), ptr(base_off, u64p), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def kernel_ms(self) -> float:
        """Milliseconds of the scan kernels of the last run(), from HIP events (rtx_chimera_kernel_time)."""
        return self._kernel_ms()


def raxtax_last_chimera() -> Tuple[int, int, int, float]:
    """rtx_raxtax_last_chimera: (queries, reads the stage checked -- the distinct ones under derep --, queries whose record is flagged, busy
    seconds of the stage) of the last raxtax() call of this process; all 0 when its handles had no chimera check set."""
    a, b, c, s = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    check(_lib.load().rtx_raxtax_last_chimera(C.byref(a), C.byref(b), C.byref(c), C.byref(s)))
    return int(a.value), int(b.value), int(c.value), float(s.value)


MERGE_MAX_READ = _lib.RTX_MERGE_MAX_READ
MG_BAD_QUALITY, MG_TOO_LONG, MG_TOO_SHORT, MG_NO_OVERLAP = (1 << b for b in range(4))


@dataclass
class MergeParams:
    """The parameters of paired-end merging (rtx_merge_params).  A candidate overlap of ov bases with d diffs scores ov - 5 d and is accepted
    iff d <= max_diffs, 100 d <= max_diff_pct * ov and the score is at least min_overlap; q_cap caps the Q of two agreeing bases."""
    ascii_base: int = 33
    min_overlap: int = 16
    max_diffs: int = 10
    max_diff_pct: int = 100
    q_cap: int = 41

    def _c(self) -> "_lib.MergeParams":
        return _lib.MergeParams(int(self.ascii_base), int(self.min_overlap), int(self.max_diffs), int(self.max_diff_pct), int(self.q_cap))


def merge_verdict_names(v: int) -> List[str]:
    """The reason of a verdict (RTX_MG_*), [] for a pair that is merged."""
    return [name for b, name in enumerate(_lib.RTX_MG_NAMES) if (int(v) >> b) & 1]


def _mate(bases, quals):
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    if len(bases) != len(quals):
        raise ValueError(f"{len(quals)} quality bytes for {len(bases)} bases")
    return bases, quals


def merge_pair(params: MergeParams, f_bases, f_quals, r_bases, r_quals) -> Tuple[int, int, int, np.ndarray, np.ndarray]:
    """rtx_merge_pair: (overlap, diffs, verdict, merged bases, merged quality bytes) of ONE pair on the host, with the functions the device
    kernel calls; the merged read is empty unless the verdict is 0."""
    fb, fq = _mate(f_bases, f_quals)
    rb, rq = _mate(r_bases, r_quals)
    one = np.zeros(1, np.uint8)
    mb, mq = (np.zeros(len(fb) + len(rb) + 1, np.uint8) for _ in range(2))
    ov, d, v, ml = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    check(_lib.load().rtx_merge_pair(C.byref(params._c()), ptr(fb if len(fb) else one, u8p), ptr(fq if len(fq) else one, u8p), len(fb),
                                     ptr(rb if len(rb) else one, u8p), ptr(rq if len(rq) else one, u8p), len(rb), C.byref(ov), C.byref(d), C.byref(v),
                                     C.byref(ml), ptr(mb, u8p), ptr(mq, u8p)))
    return int(ov.value), int(d.value), int(v.value), mb[:ml.value].copy(), mq[:ml.value].copy()


class Merge(_Stage):
    """The paired-end merging stage on one GPU (rtx_merge): an object of its own beside any Index, one stream, buffers that only grow."""

    _c = "merge"

    def __init__(self, device: int, params: MergeParams):
        self._open(device, C.byref(params._c()))

    def run(self, f_bases, f_quals, f_off, r_bases, r_quals, r_off):
        """(overlap, diffs, verdict, merged_len, merged_bases, merged_quals, slot_off) of n pairs (rtx_merge_run): the merged read of pair i
        is merged_bases[slot_off[i] : slot_off[i] + merged_len[i]], its quality bytes likewise; verdict 0: merged (merge_verdict_names)."""
        fb, fq = _mate(f_bases, f_quals)
        rb, rq = _mate(r_bases, r_quals)
        f_off = np.ascontiguousarray(f_off, dtype=np.uint64)
        r_off = np.ascontiguousarray(r_off, dtype=np.uint64)
        if len(f_off) != len(r_off) or len(f_off) < 1:
            raise ValueError(f"{len(f_off)} / {len(r_off)} offsets: the two mate arrays must describe the same number of pairs")
        n = len(f_off) - 1
        one = np.zeros(1, np.uint8)
        ov, d, v, ml = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(4))
        slot = np.zeros(n + 1, dtype=np.uint64)
        with np.errstate(over="ignore"):
            lens = (f_off[1:] - f_off[:-1]) + (r_off[1:] - r_off[:-1])
        ok = n > 0 and bool((f_off[1:] >= f_off[:-1]).all() and (r_off[1:] >= r_off[:-1]).all())
        cap = int((((lens + np.uint64(15)) // np.uint64(16)) * np.uint64(16)).sum()) if ok else 0   # (offsets that are not monotone: the call refuses them)
        mb, mq = (np.zeros(cap + 1, np.uint8) for _ in range(2))
        check(self._lib.rtx_merge_run(self._h, n, ptr(fb if len(fb) else one, u8p), ptr(fq if len(fq) else one, u8p), ptr(f_off, u64p),
                                      ptr(rb if len(rb) else one, u8p), ptr(rq if len(rq) else one, u8p), ptr(r_off, u64p), ptr(ov, u32p), ptr(d, u32p),
                                      ptr(v, u32p), ptr(ml, u32p), ptr(slot, u64p), ptr(mb, u8p), ptr(mq, u8p), cap))
        return ov[:n], d[:n], v[:n], ml[:n], mb[:cap], mq[:cap], slot

    def kernel_ms(self) -> float:
        """Milliseconds of the kernel of the last run(), from HIP events (rtx_merge_kernel_time)."""
        return self._kernel_ms()

    def stage_seconds(self) -> Tuple[float, float, float]:
        """(host staging, copies and waiting around the kernel, the whole call) of the last run(), in seconds (rtx_merge_stage_times)."""
        return self._stage_seconds()


_IUPAC_CHARS = {v: k for k, v in IUPAC.items()}


def fastq_text(records) -> str:
    """(label, bases, quals) triples as FASTQ text in the four-line form (the inverse of parse_query_fastq_str; a base code 0 has no letter)."""
    out = []
    for label, bases, quals in records:
        out.append("@%s\n%s\n+\n%s\n" % (label, "".join(_IUPAC_CHARS[int(c)] for c in bases), bytes(np.asarray(quals, np.uint8)).decode("latin-1")))
    return "".join(out)


def fastq_block_end_n(text, max_records: int) -> Tuple[int, int]:
    """rtx_fastq_block_end_n: (the offset behind the last whole record among the first max_records of the text, how many records that is)."""
    b = text.encode() if isinstance(text, str) else bytes(text)
    n = C.c_uint64()
    end = _lib.load().rtx_fastq_block_end_n(b, len(b), int(max_records), C.byref(n))
    return int(end), int(n.value)


def merge_queries(stage: Optional[Merge], fwd, rev, queries_to_skip: Sequence[str] = (), ascii_base: int = 33):
    """rtx_merge_queries: the pairs of two FASTQ inputs -- texts, or lists of (label, bases, quals) triples as parse_query_fastq_str returns
    them -- merged on the stage's GPU.  Returns ((label, bases, quals) triples ready for raxtax(..., quals=...), a pair that is not merged
    being the empty read, and the report: a list of (nf, nr, overlap, diffs, verdict) per pair)."""
    lib = _lib.load()
    texts = [(t if isinstance(t, (str, bytes)) else fastq_text(t)) for t in (fwd, rev)]
    skip = (C.c_char_p * max(len(queries_to_skip), 1))(*[s.encode() for s in queries_to_skip])
    handles = []
    try:
        for t in texts:
            b = t.encode("latin-1") if isinstance(t, str) else bytes(t)
            h = C.c_void_p()
            check(lib.rtx_queries_parse_fastq(b, len(b), None, 0, int(ascii_base), C.byref(h)))
            handles.append(h)
        m = C.c_void_p()
        check(lib.rtx_merge_queries(stage._h if stage is not None else None, handles[0], handles[1], skip, len(queries_to_skip), C.byref(m)))
        handles.append(m)
        n = lib.rtx_queries_len(m)
        p = [u32p() for _ in range(5)]
        check(lib.rtx_queries_merge_report(m, *[C.byref(x) for x in p]))
        cols = [np.ctypeslib.as_array(x, shape=(n,)).copy() if n else np.zeros(0, np.uint32) for x in p]
        return _queries_records(lib, m), [tuple(int(c[i]) for c in cols) for i in range(n)]
    finally:
        for h in handles:
            lib.rtx_queries_destroy(h)


def semiglobal_distance(q: np.ndarray, r: np.ndarray) -> int:
    """rtx_semiglobal_distance: the least Levenshtein distance between the encoded sequence q and any substring of r (the empty one
    included) -- what Result.nearest_dist holds for a query and its nearest reference, computed on the host."""
    q = np.ascontiguousarray(q, dtype=np.uint8)
    r = np.ascontiguousarray(r, dtype=np.uint8)
    d = C.c_uint32()
    one = np.zeros(1, np.uint8)
    check(_lib.load().rtx_semiglobal_distance(ptr(q if len(q) else one, u8p), len(q), ptr(r if len(r) else one, u8p), len(r), C.byref(d)))
    return int(d.value)


def revcomp(seq: np.ndarray) -> np.ndarray:
    """rtx_revcomp: the reverse complement of an encoded sequence as the library builds it."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    out = np.zeros(len(seq), dtype=np.uint8)
    check(_lib.load().rtx_revcomp(ptr(seq, u8p), len(seq), ptr(out, u8p)))
    return out


def raxtax(queries: Sequence[Tuple[str, np.ndarray]], tree, skip_exact_matches: bool, raw_confidence: bool,
           chunk_size: int, sender: Callable[[str, str, Optional[str]], None], tsv: bool,
           info: Optional[Callable[[str, int, int, int], None]] = None,
           hit: Optional[Callable[[str, int, int, int, int, int], None]] = None,
           align: Optional[Callable[[str, int, int, int, int, int, int, int], None]] = None,
           trim: Optional[Callable[[str, int, int, int, int], None]] = None,
           quals: Optional[Sequence[np.ndarray]] = None,
           qual: Optional[Callable[[str, int, int, int, int, int], None]] = None,
           chimera: Optional[Callable[[str, np.void], None]] = None,
           demux: Optional[Callable[[str, int, int, int, int, int, int], None]] = None,
           screen: Optional[Callable[[str, int, int, int, int, int], None]] = None) -> None:
    """src/raxtax.rs:14-22 -- same arguments; `tree` is the device Index built from the Tree, or a list of them (one per GPU,
    all built from the same Tree): rtx_raxtax_multi then deals the chunks to the handles, one driving thread each.
    `sender(label, out_lines, tsv_lines_or_None)` is called once per query, in input order; raising from it
    plays the role of a closed channel.  `info(label, strand, peak, t)`, if given, is called directly before the sender of the same query
    (rtx_raxtax_multi_ex); handles built with strand="both" report the orientation with the larger peak.
    `hit(label, strand, peak, t, nearest, ties)` is the same with the nearest reference and its ties (rtx_raxtax_multi_ex2; handles built with
    nearest=True, else NO_REF and 0).  `align(label, strand, peak, t, nearest, ties, dist, qlen)` adds the alignment identity
    (rtx_raxtax_multi_ex3; handles built with identity=True, else NO_DIST and the query's length).  Give one of the three.
    `trim(label, raw_len, lo, hi, hit)` is called for every query, in input order, directly before `align` (rtx_raxtax_multi_ex4; handles built
    with primers=[...]: the read kept [lo, hi) of its raw_len bases, hit as trim_hit() takes it apart); it goes with `align` or alone.
    Handles built with quality=QualParams(...) need the quality strings of the reads: queries as (label, bases, quals) triples
    (parse_query_fastq_str) or `quals`, one array per query.  `qual(label, raw_len, lo, hi, ee, verdict)` is called for every query directly
    after `trim` (rtx_raxtax_multi_ex5): the range the primers and the filter kept, the expected errors times 2^40 and the verdict (0: passed;
    qual_verdict_names); it goes with `align`, `trim` or alone.
    `chimera(label, record)` is called for every query directly after `qual` (rtx_raxtax_multi_ex6; handles built with chimera=ChimeraParams(...),
    else an empty record): the query's CHIMERA_DTYPE record -- its representative's under derep; a flagged read is classified as the empty
    read.  It goes with `align`, `trim`, `qual` or alone.
    `demux(label, raw_len, sample, lo, hi, hit, info)` is called for every query directly before `trim` (rtx_raxtax_multi_ex7; handles built with
    tags=(tags, pairs, params): the read belongs to `sample` (DEMUX_NONE: to none) and kept [lo, hi) of its raw_len bases; hit and info as
    demux_hit() takes them apart).  The callbacks behind it then speak of the cut read.  It goes with `align`, `trim`, `qual`, `chimera` or alone.
    `screen(label, windows, hits, first, source, verdict)` is called for every query directly after `qual` and before `chimera`
    (rtx_raxtax_multi_ex8; handles built with contaminants=(ScreenSet, ScreenParams), else 0, 0, SCREEN_NONE, SCREEN_NONE, 0): what the
    contaminant screen said of the range primers and quality kept; a contaminant is classified as the empty read.  It goes with the same."""
    lib = _lib.load()
    common = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), u8p, u64p, C.c_int, C.c_int, C.c_uint64, _SENDER, C.c_void_p, C.c_int]
    lib.rtx_raxtax_multi_ex7.argtypes = common + [_ALIGN, C.c_void_p, _TRIM, C.c_void_p, u8p, _QUAL, C.c_void_p, _CHIM, C.c_void_p, _DEMUX, C.c_void_p]
    lib.rtx_raxtax_multi_ex8.argtypes = lib.rtx_raxtax_multi_ex7.argtypes + [_SCREEN, C.c_void_p]
    if (info is not None) + (hit is not None) + (align is not None) > 1:
        raise ValueError("raxtax: give one of info, hit and align")
    if (trim is not None or qual is not None or chimera is not None or demux is not None or screen is not None) and (info is not None or hit is not None):
        raise ValueError("raxtax: trim, qual, chimera, demux and screen go with align or alone")
    if quals is None and info is None and hit is None and len(queries) and all(len(q) == 3 for q in queries):
        quals = [q[2] for q in queries]   # (info and hit are the callbacks of calls that carried no quality strings: triples are then read as pairs)
    if quals is not None and (info is not None or hit is not None):
        raise ValueError("raxtax: quals go with align, trim and qual")
    flat_q = None
    if quals is not None:
        if len(quals) != len(queries) or any(len(a) != len(q[1]) for a, q in zip(quals, queries)):
            raise ValueError("raxtax: quals needs one array per query, as long as its bases")
        flat_q = _flatten(list(quals))[0]
    handles = list(tree) if isinstance(tree, (list, tuple)) else [tree]
    labels = (C.c_char_p * max(len(queries), 1))(*[q[0].encode() for q in queries])
    flat, off = _flatten([q[1] for q in queries])
    err: List[BaseException] = []

    def guarded(ctype, fn, convert=lambda *a: [int(x) for x in a]):
        """fn(label, *convert(the C arguments)) as a callback of `ctype` (null for None): an exception is kept for the caller and closes the sink."""
        if fn is None and ctype is not _SENDER:
            return C.cast(None, ctype)

        def cb(_ctx, label, *args):
            try:
                fn(label.decode(), *convert(*args))
                return 0
            except BaseException as e:  # noqa: BLE001 - forwarded below
                err.append(e)
                return 1

        return ctype(cb)

    if info is not None:    # the narrower callbacks, in the shape of align
        align = lambda label, strand, peak, t, *_: info(label, strand, peak, t)  # noqa: E731
    elif hit is not None:
        align = lambda label, strand, peak, t, nearest, ties, *_: hit(label, strand, peak, t, nearest, ties)  # noqa: E731
    arr = (C.c_void_p * len(handles))(*[h._h.value for h in handles])
    rc = lib.rtx_raxtax_multi_ex8(arr, len(handles), handles[0].tree._h, len(queries), labels, ptr(flat, u8p), ptr(off, u64p),
                                  int(skip_exact_matches), int(raw_confidence), chunk_size,
                                  guarded(_SENDER, sender, lambda out, tsv_lines: (out.decode(), tsv_lines.decode() if tsv_lines is not None else None)), None, int(tsv),
                                  guarded(_ALIGN, align), None, guarded(_TRIM, trim), None, ptr(flat_q, u8p) if flat_q is not None else None,
                                  guarded(_QUAL, qual), None,
                                  guarded(_CHIM, chimera, lambda rec: [np.array([tuple(getattr(rec.contents, f) for f in _lib.RTX_CHIM_FIELDS)], CHIMERA_DTYPE)[0]]), None,
                                  guarded(_DEMUX, demux), None, guarded(_SCREEN, screen), None)
    if err:
        raise err[0]
    check(rc)


class Derep(_Stage):
    """The dereplication stage on one GPU (rtx_derep): an object of its own beside any Index, one stream, buffers that only grow."""

    _c = "derep"

    def __init__(self, device: int = 0):
        self._open(device)
        self.n_unique = 0

    def run(self, bases: np.ndarray, base_off: np.ndarray) -> np.ndarray:
        """rep[q] = the lowest query whose sequence is byte for byte that of q (rtx_derep_run); n_unique = the queries with rep[q] == q."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
        n = len(base_off) - 1
        rep = np.zeros(max(n, 1), dtype=np.uint32)
        nu = C.c_uint64()
        check(self._lib.rtx_derep_run(self._h, n, ptr(bases if len(bases) else np.zeros(1, np.uint8), u8p), ptr(base_off, u64p), ptr(rep, u32p), C.byref(nu)))
        self.n_unique = int(nu.value)
        return rep[:n]


def derep_plan(rep: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """rtx_derep_plan: (uniq, slot, size) of a dereplication map -- the queries with rep[q] == q in ascending order, the position of every
    query's representative among them, and the number of queries every one of them stands for.  RtxError if `rep` is no such map."""
    rep = np.ascontiguousarray(rep, dtype=np.uint32)
    n = len(rep)
    uniq, slot, size = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
    nu = C.c_uint64()
    check(_lib.load().rtx_derep_plan(n, ptr(rep if n else np.zeros(1, np.uint32), u32p), ptr(uniq, u32p), ptr(slot, u32p), ptr(size, u32p), C.byref(nu)))
    return uniq[:nu.value].copy(), slot[:n].copy(), size[:nu.value].copy()


def raxtax_last_derep() -> Tuple[int, int, float]:
    """rtx_raxtax_last_derep: (queries of the dereplicated chunks, distinct reads handed to the handles, busy seconds of the stage) of the
    last raxtax() call of this process; all 0 when its handles had derep off."""
    q, u, b = C.c_uint64(), C.c_uint64(), C.c_double()
    check(_lib.load().rtx_raxtax_last_derep(C.byref(q), C.byref(u), C.byref(b)))
    return int(q.value), int(u.value), float(b.value)


def _tally_args(bases, base_off, sample, weight):
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    base_off = np.ascontiguousarray(base_off, dtype=np.uint64)
    n = len(base_off) - 1
    sample = None if sample is None else np.ascontiguousarray(sample, dtype=np.uint32)
    weight = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint32)
    for name, a in (("sample", sample), ("weight", weight)):
        if a is not None and len(a) != n:
            raise ValueError(f"{len(a)} {name}s for {n} reads")
    one = np.zeros(1, np.uint32)
    return (n, ptr(bases if len(bases) else np.zeros(1, np.uint8), u8p), ptr(base_off, u64p), None if sample is None else ptr(sample if n else one, u32p),
            None if weight is None else ptr(weight if n else one, u32p)), (bases, base_off, sample, weight, one)


class TallyTable:
    """The distinct reads of a run on the host (rtx_tally_table): what Tally.read() downloads, tally_reads() accumulates and tally_merge()
    sums.  Rows sorted by total size descending, then bytes ascending.
      seqs    the rows' sequences, one uint8 code array each          counts  [rows, columns] uint64
      sizes   [rows] the sum of a row                                 first   [rows] rank in the order of first appearance
      totals  {"reads", "entries", "overflow_reads"}"""

    def __init__(self, handle):
        self._lib = _lib.load()
        self._h = handle

    def __del__(self):
        try:
            if self._h:
                self._lib.rtx_tally_table_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def add(self, bases, base_off, sample=None, weight=None) -> None:
        """rtx_tally_table_add: one more chunk into a table made by tally_reads()."""
        args, _keep = _tally_args(bases, base_off, sample, weight)
        check(self._lib.rtx_tally_table_add(self._h, *args))

    def _view(self):
        v = _lib.TallyView()
        check(self._lib.rtx_tally_table_view(self._h, C.byref(v)))
        return v

    @property
    def columns(self) -> int:
        return int(self._view().n_columns)

    @property
    def seqs(self) -> List[np.ndarray]:
        v = self._view()
        ne = int(v.n_entries)
        if ne == 0:
            return []
        off = np.ctypeslib.as_array(v.base_off, shape=(ne + 1,))
        flat = np.ctypeslib.as_array(v.bases, shape=(max(int(off[ne]), 1),))
        return [flat[int(off[r]):int(off[r + 1])].copy() for r in range(ne)]

    def _array(self, field, per_row):
        v = self._view()
        ne = int(v.n_entries)
        if ne == 0:
            return np.zeros((0, per_row) if per_row else (0,), np.uint64)
        return np.ctypeslib.as_array(getattr(v, field), shape=(ne, per_row) if per_row else (ne,)).copy()

    @property
    def counts(self) -> np.ndarray:
        return self._array("counts", self.columns)

    @property
    def sizes(self) -> np.ndarray:
        return self._array("sizes", 0)

    @property
    def first(self) -> np.ndarray:
        return self._array("first", 0)

    @property
    def totals(self) -> dict:
        v = self._view()
        return {"reads": int(v.totals[0]), "entries": int(v.totals[1]), "overflow_reads": int(v.totals[2])}

    def as_dict(self) -> dict:
        """{bytes(sequence): tuple of the row's counts}"""
        return {bytes(s): tuple(int(x) for x in c) for s, c in zip(self.seqs, self.counts)}


class Tally(_Stage):
    """The distinct reads of a run on one GPU (rtx_tally): a table that persists over any number of add() calls and owns its sequences, with
    a count per (sequence, sample).  caps: max_entries, max_bytes, initial_entries, initial_bytes (0: the header's defaults)."""

    _c = "tally"

    def __init__(self, device: int = 0, samples: int = 0, max_entries: int = 0, max_bytes: int = 0, initial_entries: int = 0, initial_bytes: int = 0):
        self.samples = int(samples)
        self._open(device, C.byref(_lib.TallyParams(self.samples, int(max_entries), int(max_bytes), int(initial_entries), int(initial_bytes))))

    def add(self, bases, base_off, sample=None, weight=None) -> None:
        """rtx_tally_add: read q adds weight[q] (None: 1) to the cell (its sequence, sample[q]) (None: column 0); a read of weight 0 or
        length 0 is not looked at."""
        args, _keep = _tally_args(bases, base_off, sample, weight)
        check(self._lib.rtx_tally_add(self._h, *args))

    def read(self) -> TallyTable:
        """rtx_tally_read: the table so far, sorted; the object goes on counting."""
        h = C.c_void_p()
        check(self._lib.rtx_tally_read(self._h, C.byref(h)))
        return TallyTable(h)

    def info(self) -> dict:
        """rtx_tally_info: entries and arena bytes in use, their capacities, and the weight counted so far."""
        v = [C.c_uint64() for _ in range(5)]
        check(self._lib.rtx_tally_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("entries", "bytes", "entry_capacity", "byte_capacity", "counted"), (int(x.value) for x in v)))


def tally_reads(bases, base_off, sample=None, weight=None, samples: int = 0) -> TallyTable:
    """rtx_tally_table_create + rtx_tally_table_add: the table of these reads accumulated on the host, without caps -- the host restatement
    of Tally.add()."""
    h = C.c_void_p()
    check(_lib.load().rtx_tally_table_create(int(samples), C.byref(h)))
    t = TallyTable(h)
    t.add(bases, base_off, sample, weight)
    return t


def tally_merge(tables: Sequence[TallyTable]) -> TallyTable:
    """rtx_tally_table_merge: the sum of tables (one Tally per handle of a multi-GPU run); equal sequences are summed."""
    arr = (C.c_void_p * len(tables))(*[t._h.value for t in tables])
    h = C.c_void_p()
    check(_lib.load().rtx_tally_table_merge(arr, len(tables), C.byref(h)))
    return TallyTable(h)


def _tally_text(fn, table, *args) -> str:
    n = check(fn(table._h, *args, None, 0))
    buf = C.create_string_buffer(max(n, 1))
    check(fn(table._h, *args, buf, n))
    return buf.raw[:n].decode()


def tally_fasta(table: TallyTable, minsize: int = 1) -> str:
    """rtx_tally_format_fasta: `>uniq{rank};size={N}` and the sequence per row (what raxtax-hip --uniques writes to PREFIX/raxtax.uniques)."""
    return _tally_text(_lib.load().rtx_tally_format_fasta, table, int(minsize))


def tally_table_text(table: TallyTable, names: Sequence[str], minsize: int = 1) -> str:
    """rtx_tally_format_table: the sequence x sample table of read counts (PREFIX/raxtax.uniques.tsv); one name per column."""
    if len(names) != table.columns:
        raise ValueError(f"{len(names)} names for {table.columns} column(s)")
    arr = (C.c_char_p * len(names))(*[s.encode() for s in names])
    return _tally_text(_lib.load().rtx_tally_format_table, table, arr, int(minsize))


class Otus:
    """The OTUs of a run (rtx_otu): the rows of a TallyTable clustered by Swarm's d = 1 rule, by otu_cluster() on a GPU or otu_cluster_host().
      otu      [rows] the OTU of a row, from 0 in the order of the seeds       seed     [otus] the rank of the seed
      members  [otus] rows                                                     sizes    [otus] the sum of the counts
      counts   [otus, columns]                                                 links    [n, 2] the linked rows (a, b), a < b, sorted
      rounds, link_passes (the device's), long_rows (rows above RTX_OTU_MAX_LEN: no links)
      seconds  upload, link passes, labels and numbering, download of a device run"""

    def __init__(self, handle, table: "TallyTable"):
        self._lib = _lib.load()
        self._h = handle
        self.table = table   # (the formatters read the seeds' sequences from it)
        v = _lib.OtuView()
        check(self._lib.rtx_otu_view(self._h, C.byref(v)))
        nr, no, nl, nc = int(v.n_rows), int(v.n_otus), int(v.n_links), int(v.n_columns)

        def arr(p, n, dtype, shape=None):
            if n == 0:
                return np.zeros(shape if shape else (0,), dtype)
            return np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(shape if shape else (n,))

        self.n_rows, self.n_otus, self.columns = nr, no, nc
        self.otu = arr(v.otu, nr, np.uint32)
        self.seed = arr(v.seed, no, np.uint32)
        self.members = arr(v.members, no, np.uint64)
        self.sizes = arr(v.sizes, no, np.uint64)
        self.counts = arr(v.counts, no * nc, np.uint64, (no, nc))
        self.links = np.stack([arr(v.link_a, nl, np.uint32), arr(v.link_b, nl, np.uint32)], axis=1)
        self.rounds, self.link_passes, self.long_rows = int(v.rounds), int(v.link_passes), int(v.long_rows)
        t = (C.c_double * 4)()
        check(self._lib.rtx_otu_times(self._h, t))
        self.seconds = tuple(float(x) for x in t)

    def _read_graft(self):
        """what a graft result carries beside its clustering (otu_graft, otu_graft_host): parent [rows], old_to_new [old otus], grafts [n, 5]
        (old light OTU, child row, parent row, old heavy OTU, new number; sorted by the first) and graft_info, the counters"""
        g = _lib.GraftView()
        check(self._lib.rtx_otu_graft_view(self._h, C.byref(g)))

        def arr(p, n):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)

        ng = int(g.n_grafts)
        self.parent = arr(g.parent, int(g.n_rows))
        self.old_to_new = arr(g.old_to_new, int(g.n_old_otus))
        self.grafts = np.stack([arr(p, ng) for p in (g.light, g.child, g.par, g.heavy, g.into)], axis=1)
        self.graft_info = {k: int(getattr(g, k)) for k in ("boundary", "heavy_otus", "light_otus", "heavy_rows", "light_rows", "variants", "candidates", "confirmed",
                                                            "bloom_log2", "test_passes")}
        self.graft_info["grafts"] = ng
        self.graft_info["seconds"] = tuple(float(x) for x in g.seconds)
        return self

    def _read_unoise(self):
        """what a denoising result carries beside its clustering (otu_unoise, otu_unoise_host): .unoise, the view as numpy arrays -- status
        (_lib.RTX_UNOISE_*), parent (NO_REF: none), dist (NO_DIST: none) and lim per row, the four status counts, the parameters as used, the
        device's counters (0 from the host) and the seconds of upload, pair kernels, bookkeeping and download"""
        g = _lib.UnoiseView()
        check(self._lib.rtx_otu_unoise_view(self._h, C.byref(g)))
        n = int(g.n_rows)

        def arr(p, dtype):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype)

        self.unoise = {"status": arr(g.status, np.uint8), "parent": arr(g.parent, np.uint32), "dist": arr(g.dist, np.uint32), "lim": arr(g.lim, np.uint32)}
        self.unoise.update({k: int(getattr(g, k)) for k in ("n_zotu", "n_absorbed", "n_left", "n_long", "minsize", "alpha", "max_diffs", "tiers", "launches", "pairs",
                                                            "pairs_length", "pairs_finished")})
        self.unoise["seconds"] = tuple(float(x) for x in g.seconds)
        return self

    def __del__(self):
        try:
            if self._h:
                self._lib.rtx_otu_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _otu_params(differences: int = 1, flags: int = 0, initial_links: int = 0):
    return C.byref(_lib.OtuParams(int(differences), int(flags), int(initial_links)))


def otu_cluster(table: TallyTable, device: int = 0, **params) -> Otus:
    """rtx_otu_cluster: the OTUs of the table's rows, on GPU `device`.  params: differences (1), flags (0), initial_links (0: a default)."""
    h = C.c_void_p()
    check(_lib.load().rtx_otu_cluster(int(device), table._h, _otu_params(**params), C.byref(h)))
    return Otus(h, table)


def otu_cluster_host(table: TallyTable, **params) -> Otus:
    """rtx_otu_cluster_host: the same from the definition, on the host."""
    h = C.c_void_p()
    check(_lib.load().rtx_otu_cluster_host(table._h, _otu_params(**params), C.byref(h)))
    return Otus(h, table)


def _otu_text(fn, otus, *args) -> str:
    n = check(fn(otus._h, *args, None, 0))
    buf = C.create_string_buffer(max(n, 1))
    check(fn(otus._h, *args, buf, n))
    return buf.raw[:n].decode()


def otu_fasta(otus: Otus, minsize: int = 1) -> str:
    """rtx_otu_format_fasta: `>otu{k};size={N};seed=uniq{rank}` and the seed's sequence per OTU (PREFIX/raxtax.otus of raxtax-hip --otus)."""
    return _otu_text(_lib.load().rtx_otu_format_fasta, otus, otus.table._h, int(minsize))


def otu_table_text(otus: Otus, names: Sequence[str], minsize: int = 1) -> str:
    """rtx_otu_format_table: the OTU x sample table of read counts (PREFIX/raxtax.otus.tsv); one name per column."""
    if len(names) != otus.columns:
        raise ValueError(f"{len(names)} names for {otus.columns} column(s)")
    arr = (C.c_char_p * len(names))(*[s.encode() for s in names])
    return _otu_text(_lib.load().rtx_otu_format_table, otus, arr, int(minsize))


def otu_map_text(otus: Otus) -> str:
    """rtx_otu_format_map: `uniq{rank}\totu{k}` per row of the table (PREFIX/raxtax.otus.map)."""
    return _otu_text(_lib.load().rtx_otu_format_map, otus)


def _graft_params(boundary: int = 0, bloom_log2: int = 0, flags: int = 0, max_bloom_bytes: int = 0, initial_candidates: int = 0):
    return C.byref(_lib.GraftParams(int(boundary), int(bloom_log2), int(flags), int(max_bloom_bytes), int(initial_candidates)))


def otu_graft(otus: Otus, device: int = 0, **params) -> Otus:
    """rtx_otu_graft: Swarm's fastidious pass on GPU `device` -- the OTUs of `otus` below the boundary grafted onto an OTU at or above it that
    holds a row at most two differences away.  A new Otus over the same table, with .parent, .old_to_new, .grafts and .graft_info.
    params: boundary (0: 3), bloom_log2 (0: from the heavy rows), flags (0), max_bloom_bytes (0: 8 GiB), initial_candidates (0: a default)."""
    h = C.c_void_p()
    check(_lib.load().rtx_otu_graft(int(device), otus.table._h, otus._h, _graft_params(**params), C.byref(h)))
    return Otus(h, otus.table)._read_graft()


def otu_graft_host(otus: Otus, **params) -> Otus:
    """rtx_otu_graft_host: the same from the definition, on the host (the filter's counters stay 0)."""
    h = C.c_void_p()
    check(_lib.load().rtx_otu_graft_host(otus.table._h, otus._h, _graft_params(**params), C.byref(h)))
    return Otus(h, otus.table)._read_graft()


def otu_grafts_text(otus: Otus) -> str:
    """rtx_otu_format_grafts: `otu{k}\t{size}\tuniq{child}\tuniq{parent}\totu{heavy}\totu{new}` per graft (PREFIX/raxtax.otus.grafts)."""
    return _otu_text(_lib.load().rtx_otu_format_grafts, otus)


@dataclass
class UnoiseParams:
    """rtx_unoise_params: minsize (a ZOTU holds at least that many reads), alpha (the skew exponent, 1 .. 8), max_diffs (0: 16), flags (0)."""
    minsize: int = 8
    alpha: int = 2
    max_diffs: int = 0
    flags: int = 0

    def _c(self):
        return C.byref(_lib.UnoiseParams(int(self.minsize), int(self.alpha), int(self.max_diffs), int(self.flags)))


def otu_unoise(table: TallyTable, device: int = 0, **params) -> Otus:
    """rtx_otu_unoise: the table's rows denoised into ZOTUs by the UNOISE rule, on GPU `device`.  An Otus over the table -- every row that is not
    absorbed seeds an OTU -- with .unoise.  params: the fields of UnoiseParams."""
    h = C.c_void_p()
    check(_lib.load().rtx_otu_unoise(int(device), table._h, UnoiseParams(**params)._c(), C.byref(h)))
    return Otus(h, table)._read_unoise()


def otu_unoise_host(table: TallyTable, **params) -> Otus:
    """rtx_otu_unoise_host: the same from the definition, on the host (the device's counters stay 0)."""
    h = C.c_void_p()
    check(_lib.load().rtx_otu_unoise_host(table._h, UnoiseParams(**params)._c(), C.byref(h)))
    return Otus(h, table)._read_unoise()


def unoise_text(otus: Otus) -> str:
    """rtx_otu_format_unoise: `uniq{rank}\t{size}\t{status}\t{parent}\t{diffs}\totu{k}` per row (PREFIX/raxtax.otus.unoise)."""
    return _otu_text(_lib.load().rtx_otu_format_unoise, otus)


@dataclass
class Lineages:
    """The records of a batch (rtx_lineage_records): per query what the taxon profile takes of it under a cutoff -- kind (_lib.RTX_LIN_*),
    L (the leading levels of its best lineage that reach the cutoff), node (a_{L-1}) and hund [n, stride] (their hundredths, 0 from L on)."""
    kind: np.ndarray
    L: np.ndarray
    node: np.ndarray
    hund: np.ndarray

    def __len__(self) -> int:
        return len(self.kind)

    def _c(self) -> "_lib.LineageRecords":
        self.kind = np.ascontiguousarray(self.kind, dtype=np.uint8)
        self.L = np.ascontiguousarray(self.L, dtype=np.uint8)
        self.node = np.ascontiguousarray(self.node, dtype=np.uint32)
        h = np.ascontiguousarray(self.hund, dtype=np.uint8)
        self.hund = h.reshape(len(self.kind), -1) if len(self.kind) else h.reshape(0, max(1, h.shape[-1]))
        return _lib.LineageRecords(ptr(self.kind, u8p), ptr(self.L, u8p), ptr(self.node, u32p), ptr(self.hund, u8p), int(self.hund.shape[1]))

    @staticmethod
    def concat(parts: Sequence["Lineages"]) -> "Lineages":
        return Lineages(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("kind", "L", "node", "hund")))


def best_lineages(tree: Tree, result: Result, cutoff: int = 80, skip_exact_matches: bool = False, raw_confidence: bool = False, exact=None) -> Lineages:
    """rtx_result_best_lineages: the records of a classified batch, by the per-query step of the taxon profile.  cutoff in hundredths (1 .. 100);
    exact = (ids, off), the exact matches of the batch (Index.exact_matches), or None: no query has one."""
    nq, nr = int(result.n_queries), len(result.row_node)
    stride = int(result.row_conf.shape[1]) if result.row_conf.ndim == 2 else RTX_MAX_DEPTH
    keep = dict(t=np.ascontiguousarray(result.t, np.uint32), status=np.ascontiguousarray(result.status, np.uint8),
                gs=np.ascontiguousarray(result.global_signal, np.float64), begin=np.ascontiguousarray(result.row_off[:-1], np.uint64),
                count=np.ascontiguousarray(np.diff(result.row_off.astype(np.int64)), np.uint32), lin=np.ascontiguousarray(result.row_lineage, np.uint32),
                node=np.ascontiguousarray(result.row_node, np.uint32), depth=np.ascontiguousarray(result.row_depth, np.uint32),
                conf=np.ascontiguousarray(result.row_conf, np.float64), local=np.ascontiguousarray(result.row_local_signal, np.float64),
                depth8=np.ascontiguousarray(result.row_depth, np.uint8), hund=np.ascontiguousarray(result.row_conf_hundredths, np.uint8))
    view = ResultView(nq, nr, ptr(keep["t"], u32p), ptr(keep["status"], u8p), ptr(keep["gs"], f64p), ptr(keep["begin"], u64p), ptr(keep["count"], u32p),
                      ptr(keep["lin"], u32p), ptr(keep["node"], u32p), ptr(keep["depth"], u32p), ptr(keep["conf"], f64p), ptr(keep["local"], f64p),
                      stride, ptr(keep["depth8"], u8p), ptr(keep["hund"], u8p))
    ids = off = None
    if exact is not None:
        ids = np.ascontiguousarray(exact[0], np.uint32)
        off = np.ascontiguousarray(exact[1], np.uint64)
        if len(ids) == 0:
            ids = np.zeros(1, np.uint32)
    flags = (RTX_SKIP_EXACT_MATCHES if skip_exact_matches else 0) | (RTX_RAW_CONFIDENCE if raw_confidence else 0)
    hs = max(stride, 1)
    out = Lineages(np.zeros(nq, np.uint8), np.zeros(nq, np.uint8), np.zeros(nq, np.uint32), np.zeros((nq, hs), np.uint8))
    check(_lib.load().rtx_result_best_lineages(tree._h, C.byref(view), None if ids is None else ptr(ids, u32p), None if off is None else ptr(off, u64p),
                                               int(cutoff), flags, ptr(out.kind, u8p), ptr(out.L, u8p), ptr(out.node, u32p), ptr(out.hund, u8p), hs))
    return out


class OtuTaxonomy:
    """The consensus taxonomy of the OTUs (rtx_otu_taxonomy / rtx_otu_taxonomy_host): per OTU sizes, members, classified, depth, node, seed_rel
    (0 equal, 1 the consensus is a prefix of the seed's path, 2 the other way round, 3 they diverge) and clade, conf [otus, stride]; agree_pct;
    packed_waves, big_otus (the device's plan) and seconds (checks, plan and upload; path kernel; consensus kernels; download)."""

    def __init__(self, handle):
        self._lib = _lib.load()
        self._h = handle
        v = _lib.OtuTaxonomyView()
        check(self._lib.rtx_otu_taxonomy_view(self._h, C.byref(v)))
        no, st = int(v.n_otus), int(v.stride)

        def arr(p, n, dtype, shape=None):
            if n == 0:
                return np.zeros(shape if shape else (0,), dtype)
            return np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(shape if shape else (n,))

        self.n_rows, self.n_otus, self.n_nodes, self.agree_pct, self.stride = int(v.n_rows), no, int(v.n_nodes), int(v.agree_pct), st
        self.sizes = arr(v.sizes, no, np.uint64)
        self.members = arr(v.members, no, np.uint64)
        self.classified = arr(v.classified, no, np.uint64)
        self.depth = arr(v.depth, no, np.uint32)
        self.node = arr(v.node, no, np.uint32)
        self.seed_rel = arr(v.seed_rel, no, np.uint8)
        self.clade = arr(v.clade, no * st, np.uint64, (no, st))
        self.conf = arr(v.conf, no * st, np.uint64, (no, st))
        self.packed_waves, self.big_otus = int(v.packed_waves), int(v.big_otus)
        t = (C.c_double * 4)()
        check(self._lib.rtx_otu_taxonomy_times(self._h, t))
        self.seconds = tuple(float(x) for x in t)

    def text(self, tree: Tree, minsize: int = 0) -> str:
        """rtx_otu_taxonomy_format: a header line and one line per OTU whose size reaches minsize (PREFIX/raxtax.otus.tax of raxtax-hip --otus-tax)."""
        fn = self._lib.rtx_otu_taxonomy_format
        n = check(fn(self._h, tree._h, int(minsize), None, 0))
        buf = C.create_string_buffer(max(n, 1))
        check(fn(self._h, tree._h, int(minsize), buf, n))
        return buf.raw[:n].decode()

    def __del__(self):
        try:
            if self._h:
                self._lib.rtx_otu_taxonomy_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _otutax_args(tree, otus, lineages, agree):
    """otus: an Otus object, or (otu [rows], weight [rows], seed [otus]); tree: a Tree, or the parent array of its nodes"""
    if isinstance(otus, Otus):
        otu, weight, seed = otus.otu, otus.table.sizes, otus.seed
    else:
        otu, weight, seed = otus
    otu = np.ascontiguousarray(otu, np.uint32)
    weight = np.ascontiguousarray(weight, np.uint64)
    seed = np.ascontiguousarray(seed, np.uint32)
    if len(weight) != len(otu) or len(lineages) != len(otu):
        raise ValueError(f"{len(otu)} rows, {len(weight)} weights, {len(lineages)} records")
    parent = np.ascontiguousarray(tree.nodes()["parent"] if isinstance(tree, Tree) else tree, np.uint32)
    nodes = NodesView(len(parent), None, None, None, None, ptr(parent, u32p), None)
    keep = (otu, weight, seed, parent, lineages)
    return keep, (len(otu), ptr(otu, u32p), ptr(weight, u64p), len(seed), ptr(seed, u32p), C.byref(lineages._c()), C.byref(nodes),
                  C.byref(_lib.OtuTaxonomyParams(int(agree), 0)))


def otu_taxonomy(tree, otus, lineages: Lineages, device: int = 0, agree: int = 51) -> OtuTaxonomy:
    """rtx_otu_taxonomy on GPU `device`: per OTU the deepest taxon that `agree` percent (51 .. 100) of its reads reach, with the support of every level."""
    keep, args = _otutax_args(tree, otus, lineages, agree)
    h = C.c_void_p()
    check(_lib.load().rtx_otu_taxonomy(int(device), *args, C.byref(h)))
    return OtuTaxonomy(h)


def otu_taxonomy_host(tree, otus, lineages: Lineages, agree: int = 51) -> OtuTaxonomy:
    """rtx_otu_taxonomy_host: the same from the definition, on the host."""
    keep, args = _otutax_args(tree, otus, lineages, agree)
    h = C.c_void_p()
    check(_lib.load().rtx_otu_taxonomy_host(*args, C.byref(h)))
    return OtuTaxonomy(h)


class DenovoParams:
    """rtx_denovo_params: segments S (2 .. 32) and mindelta as ChimeraParams, abskew (an integer >= 1: a parent is at least abskew times as
    abundant as the entry), max_parents (0: the default, 262 144, which is also the most), flags (0)."""

    def __init__(self, segments: int = 16, mindelta: int = 24, abskew: int = _lib.RTX_DENOVO_DEFAULT_ABSKEW, max_parents: int = 0, flags: int = 0):
        self.segments, self.mindelta, self.abskew, self.max_parents, self.flags = int(segments), int(mindelta), int(abskew), int(max_parents), int(flags)

    def _c(self):
        return C.byref(_lib.DenovoParams(self.segments, self.mindelta, self.abskew, self.max_parents, self.flags))


class Denovo:
    """The de novo chimera check of a run (rtx_denovo), by denovo_check() on a GPU or denovo_check_host().
      row      [entries] the table rank of an entry          otu     [entries] its OTU, or None without an Otus object
      weight   [entries]                                     lim     [entries] the entries below it are its candidate parents
      rec      [entries] structured array of the twelve fields of rtx_chimera_rec; parents are entry indices
      n_checked, n_flagged, rounds, scans; seconds: upload and bitmap, scans, the rounds' bookkeeping, download of a device run"""

    def __init__(self, handle, table: "TallyTable", otus: Optional["Otus"]):
        self._lib = _lib.load()
        self._h = handle
        self.table, self.otus = table, otus   # (the formatters read them)
        v = _lib.DenovoView()
        check(self._lib.rtx_denovo_view(self._h, C.byref(v)))
        n = int(v.n_entries)

        def arr(p, dtype):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype)

        self.n_entries = n
        self.row = arr(v.row, np.uint32)
        self.otu = arr(v.otu, np.uint32) if v.otu else None
        self.weight = arr(v.weight, np.uint64)
        self.lim = arr(v.lim, np.uint32)
        dt = np.dtype([(f, np.uint32) for f in _lib.RTX_CHIM_FIELDS])
        self.rec = np.frombuffer(C.string_at(v.rec, n * 48), dtype=dt).copy() if n else np.zeros(0, dt)
        self.n_checked, self.n_flagged, self.rounds, self.scans = int(v.n_checked), int(v.n_flagged), int(v.rounds), int(v.scans)
        t = (C.c_double * 4)()
        check(self._lib.rtx_denovo_times(self._h, t))
        self.seconds = tuple(float(x) for x in t)

    def __del__(self):
        try:
            if self._h:
                self._lib.rtx_denovo_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _denovo_params(params):
    p = params.pop("params", None)
    if p is not None and params:
        raise TypeError("either params or keyword parameters")
    return (p if p is not None else DenovoParams(**params))._c()


def denovo_check(table: TallyTable, otus: Optional[Otus] = None, device: int = 0, **params) -> Denovo:
    """rtx_denovo_check: the de novo chimera check of the table's rows, or of the seeds of `otus` (made from this table), on GPU `device`.
    params: those of DenovoParams, or params=DenovoParams(...)."""
    h = C.c_void_p()
    check(_lib.load().rtx_denovo_check(int(device), table._h, otus._h if otus is not None else None, _denovo_params(params), C.byref(h)))
    return Denovo(h, table, otus)


def denovo_check_host(table: TallyTable, otus: Optional[Otus] = None, **params) -> Denovo:
    """rtx_denovo_check_host: the same from the definition, on the host."""
    h = C.c_void_p()
    check(_lib.load().rtx_denovo_check_host(table._h, otus._h if otus is not None else None, _denovo_params(params), C.byref(h)))
    return Denovo(h, table, otus)


def _denovo_text(fn, d, *args) -> str:
    n = check(fn(d._h, *args, None, 0))
    buf = C.create_string_buffer(max(n, 1))
    check(fn(d._h, *args, buf, n))
    return buf.raw[:n].decode()


def denovo_records_text(d: Denovo) -> str:
    """rtx_denovo_format_records: a header line and one line per entry (PREFIX/raxtax.otus.denovo of raxtax-hip --denovo)."""
    return _denovo_text(_lib.load().rtx_denovo_format_records, d)


def denovo_fasta(d: Denovo, minsize: int = 1) -> str:
    """rtx_denovo_format_fasta: the lines of otu_fasta() / tally_fasta() of the entries that are not flagged (PREFIX/raxtax.otus.clean)."""
    return _denovo_text(_lib.load().rtx_denovo_format_fasta, d, d.table._h, d.otus._h if d.otus is not None else None, int(minsize))


def denovo_table_text(d: Denovo, names: Sequence[str], minsize: int = 1) -> str:
    """rtx_denovo_format_table: the same selection of otu_table_text() / tally_table_text() (PREFIX/raxtax.otus.clean.tsv)."""
    if len(names) != d.table.columns:
        raise ValueError(f"{len(names)} names for {d.table.columns} column(s)")
    arr = (C.c_char_p * len(names))(*[s.encode() for s in names])
    return _denovo_text(_lib.load().rtx_denovo_format_table, d, d.table._h, d.otus._h if d.otus is not None else None, arr, int(minsize))


def raxtax_last_tally() -> Tuple[int, int, int, float]:
    """rtx_raxtax_last_tally: (queries of the tallied chunks, those that counted, entries the objects gained, busy seconds of the stage) of
    the last raxtax() call of this process; all 0 when its handles had no tally."""
    q, c, a, b = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    check(_lib.load().rtx_raxtax_last_tally(C.byref(q), C.byref(c), C.byref(a), C.byref(b)))
    return int(q.value), int(c.value), int(a.value), float(b.value)


def raxtax_last_timing() -> Tuple[List[float], int]:
    """rtx_raxtax_last_timing: busy seconds of the pipeline stages (host lookup, device, format, sender) and the number of chunks of the
    last rtx_raxtax / rtx_raxtax_multi call of this process."""
    lib = _lib.load()
    busy = (C.c_double * 4)()
    n_chunks = C.c_uint64(0)
    check(lib.rtx_raxtax_last_timing(busy, C.byref(n_chunks)))
    return [float(b) for b in busy], int(n_chunks.value)
