"""ctypes binding of include/kmersets_hip.h (libkmersets_hip.so, HIP/gfx950).

Device memory is owned by torch tensors (plumbing); the C ABI only ever sees raw
device pointers.  There is no CPU fallback: if the library is missing or no GPU is
visible, calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(CSRC_DIR, "libkmersets_hip.so")
ROOT = os.path.dirname(PKG_DIR)
HEADER = os.path.join(ROOT, "include", "kmersets_hip.h")

KSH_OK, KSH_INVALID_ARGUMENT, KSH_FAILED_PRECONDITION, KSH_INTERNAL = 0, 3, 9, 13


class KshError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("ksh error %d: %s" % (code, message))
        self.code = code


class Geom(C.Structure):
    _fields_ = [("k", C.c_int32), ("n_bucket_bits", C.c_int32), ("key_bytes", C.c_int32),
                ("reserved", C.c_int32)]


class SetView(C.Structure):
    _fields_ = [("d_offsets", C.c_void_p), ("d_keys", C.c_void_p), ("n_keys", C.c_int64)]


class SpssView(C.Structure):
    _fields_ = [("d_words", C.c_void_p), ("d_lens", C.c_void_p), ("n_strings", C.c_int64),
                ("n_bases", C.c_int64)]


GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64))
COMM_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
COMM_P2P_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32)
KSH_COMM_ID_BYTES = 128


COMM_ABORT_FN = C.CFUNCTYPE(None, C.c_void_p)


class CommFns(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("user", C.c_void_p), ("allgather", COMM_ALLGATHER_FN), ("send", COMM_P2P_FN),
                ("recv", COMM_P2P_FN), ("abort", COMM_ABORT_FN)]


class PairJob(C.Structure):
    _fields_ = [("a", SetView), ("b", SetView), ("d_off_i", C.c_void_p), ("d_off_amb", C.c_void_p),
                ("d_off_bma", C.c_void_p), ("d_keys_i", C.c_void_p), ("d_keys_amb", C.c_void_p),
                ("d_keys_bma", C.c_void_p), ("totals", C.c_int64 * 3)]


class Selection(C.Structure):
    """ksh_kss_selection; the lists are host arrays of int32 node ids."""
    _fields_ = [("struct_size", C.c_size_t), ("cols", C.POINTER(C.c_int32)), ("n_cols", C.c_int32),
                ("min_count", C.c_int32), ("max_count", C.c_int32), ("require", C.POINTER(C.c_int32)),
                ("n_require", C.c_int32), ("exclude", C.POINTER(C.c_int32)), ("n_exclude", C.c_int32)]


class LinkGraph(C.Structure):
    """ksh_link_graph; the link arrays and the classes are device pointers, rows is a host array."""
    _fields_ = [("struct_size", C.c_size_t), ("n_strings", C.c_int64), ("d_link_offsets", C.c_void_p),
                ("d_link_to", C.c_void_p), ("n_links", C.c_int64), ("d_string_class", C.c_void_p),
                ("rows", C.POINTER(C.c_uint64)), ("n_classes", C.c_int64)]


class LocateReq(C.Structure):
    """ksh_seq_locate_req; the views are host structs of device pointers, the outputs device pointers."""
    _fields_ = [("struct_size", C.c_size_t), ("ctx", C.c_void_p), ("g", C.POINTER(Geom)),
                ("strings", C.POINTER(SpssView)), ("reference", C.POINTER(SpssView)), ("canonical", C.c_int32),
                ("d_where", C.c_void_p), ("d_count", C.c_void_p), ("n_located", C.POINTER(C.c_int64))]


class SeqPaint(C.Structure):
    """ksh_seq_paint; cols and rows are host arrays."""
    _fields_ = [("struct_size", C.c_size_t), ("cols", C.POINTER(C.c_int32)), ("n_cols", C.c_int32),
                ("canonicalize", C.c_int32), ("rows", C.POINTER(C.c_uint64)), ("n_classes", C.c_int64),
                ("route", C.c_int32), ("pass_positions", C.c_int64)]


def build(force=False):
    """Compiles the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC_DIR, f) for f in os.listdir(CSRC_DIR) if f.endswith((".hip", ".h"))]
    srcs.append(HEADER)
    if force or not os.path.exists(LIB_PATH) or any(
            os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-C", CSRC_DIR, "-s", "-j4"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("KSH_LIB") or LIB_PATH   # KSH_LIB: another build of the same sources (tools/probe_trace.py)
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is missing: run __graft_entry__.build() (make -C %s). "
            "The k-mer set hot path has no CPU fallback." % (path, CSRC_DIR))
    # torch ships its own libamdhip64; load it first so that this library binds to the
    # same HIP runtime (two runtimes in one process cannot both open the device).
    import torch  # noqa: F401

    L = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    GP, SP = C.POINTER(Geom), C.POINTER(SetView)
    sig = {
        "ksh_version": (C.c_int, []),
        "ksh_last_error": (C.c_char_p, []),
        "ksh_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "ksh_malloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(vp)]),
        "ksh_free": (C.c_int, [C.c_int, vp]),
        "ksh_memcpy_h2d": (C.c_int, [C.c_int, vp, vp, C.c_size_t]),
        "ksh_memcpy_d2h": (C.c_int, [C.c_int, vp, vp, C.c_size_t]),
        "ksh_memcpy_d2d": (C.c_int, [C.c_int, vp, vp, C.c_size_t]),
        "ksh_ctx_memcpy_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "ksh_ctx_memcpy_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "ksh_ctx_memcpy_d2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
        "ksh_ctx_create": (C.c_int, [C.c_int, vp, C.POINTER(vp)]),
        "ksh_ctx_destroy": (C.c_int, [vp]),
        "ksh_ctx_sync": (C.c_int, [vp]),
        "ksh_ctx_reserve": (C.c_int, [vp, C.c_size_t]),
        "ksh_ctx_enable_timing": (C.c_int, [vp, C.c_int]),
        "ksh_ctx_timing_reset": (C.c_int, [vp]),
        "ksh_ctx_timing_read": (C.c_int, [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(i64)]),
        "ksh_ctx_timing_units": (C.c_int, [vp, C.c_int, C.POINTER(i64)]),
        "ksh_ctx_set_lanes": (C.c_int, [vp, C.c_int]),
        "ksh_ctx_mem_stats": (C.c_int, [vp, C.POINTER(i64), C.c_int]),
        "ksh_ctx_timing_wall": (C.c_int, [vp, C.c_int, C.POINTER(C.c_float)]),
        "ksh_set_hash": (C.c_int, [vp, GP, SP, C.POINTER(C.c_uint64)]),
        "ksh_dsu_components": (C.c_int, [vp, i64, vp, vp, i64, vp]),
        "ksh_set_contains": (C.c_int, [vp, GP, SP, vp, i64, vp]),
        "ksh_set_kmers": (C.c_int, [vp, GP, SP, vp]),
        "ksh_pair_plan": (C.c_int, [vp, GP, SP, SP, vp, vp, vp, C.POINTER(i64)]),
        "ksh_pair_write": (C.c_int, [vp, GP, SP, SP, vp, vp, vp]),
        "ksh_set_diff": (C.c_int, [vp, GP, SP, SP, C.POINTER(i64)]),
        "ksh_pair_algebra": (C.c_int, [vp, GP, SP, SP, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]),
        "ksh_pair_algebra_batch": (C.c_int, [vp, GP, C.POINTER(PairJob), i32]),
        "ksh_pair_weights": (C.c_int, [vp, GP, SP, i32, C.POINTER(i32), i32, C.POINTER(i32), i32,
                                       C.POINTER(i64)]),
        "ksh_spss_size": (C.c_int, [vp, GP, C.POINTER(SpssView), C.POINTER(i64)]),
        "ksh_spss_decode_plan": (C.c_int, [vp, GP, C.POINTER(SpssView), C.c_int, vp, C.POINTER(i64)]),
        "ksh_spss_decode_write": (C.c_int, [vp, GP, C.POINTER(SpssView), C.c_int, vp, vp,
                                            C.POINTER(i64)]),
        "ksh_fasta_plan": (C.c_int, [vp, GP, vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        "ksh_fasta_write": (C.c_int, [vp, vp, vp]),
        "ksh_fasta_write_for": (C.c_int, [vp, vp, vp, i64, i64, vp]),
        "ksh_kmer_count_write": (C.c_int, [vp, GP, C.POINTER(SpssView), C.c_int, i32, vp, vp, C.POINTER(i64),
                                           C.POINTER(i64)]),
        "ksh_spss_to_text": (C.c_int, [vp, GP, C.POINTER(SpssView), vp]),
        "ksh_spss_from_text_plan": (C.c_int, [vp, GP, vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        "ksh_spss_from_text_write": (C.c_int, [vp, vp, vp]),
        "ksh_spss_from_text_write_for": (C.c_int, [vp, vp, vp, i64, i64, vp]),
        "ksh_spss_encode_plan": (C.c_int, [vp, GP, SP, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]),
        "ksh_spss_encode_write": (C.c_int, [vp, vp, vp]),
        "ksh_spss_encode_write_for": (C.c_int, [vp, vp, vp, i64, i64, vp]),
        "ksh_spss_encode_stats": (C.c_int, [vp, C.POINTER(i64)]),
        "ksh_spss_encode_routes": (C.c_int, [vp, C.POINTER(i64)]),
        "ksh_spss_encode_release": (C.c_int, [vp]),
        "ksh_spss_cover_plan": (C.c_int, [vp, GP, C.POINTER(SpssView), C.c_int, C.c_int, C.POINTER(i64),
                                          C.POINTER(i64)]),
        "ksh_spss_cover_write": (C.c_int, [vp, vp, vp]),
        "ksh_spss_cover_write_for": (C.c_int, [vp, vp, vp, i64, i64, vp]),
        "ksh_spss_cover_stats": (C.c_int, [vp, C.POINTER(i64)]),
        "ksh_spss_cover_release": (C.c_int, [vp]),
        "ksh_set_union_plan": (C.c_int, [vp, GP, SP, SP, vp, C.POINTER(i64)]),
        "ksh_set_union_write": (C.c_int, [vp, GP, SP, SP, vp]),
        "ksh_svb_encode_0124": (C.c_int, [vp, vp, i64, vp, C.POINTER(i64)]),
        "ksh_svb_decode_0124": (C.c_int, [vp, vp, i64, vp, C.POINTER(i64)]),
        "ksh_kss_build": (C.c_int, [vp, GP, C.POINTER(SpssView), i32, C.POINTER(i32), i32, C.c_int,
                                    i32, C.POINTER(vp)]),
        "ksh_kss_build_sharded": (C.c_int, [vp, GP, C.POINTER(SpssView), i32, C.POINTER(i32), i32, C.c_int,
                                            i32, i32, i32, GATHER_FN, vp, C.POINTER(vp)]),
        "ksh_kss_node_holder": (C.c_int, [vp, i32, C.POINTER(i32)]),
        "ksh_comm_unique_id": (C.c_int, [C.c_char_p]),
        "ksh_comm_create_rccl": (C.c_int, [vp, i32, i32, C.c_char_p, C.POINTER(vp)]),
        "ksh_comm_create_custom": (C.c_int, [vp, i32, i32, C.POINTER(CommFns), C.POINTER(vp)]),
        "ksh_comm_destroy": (C.c_int, [vp]),
        "ksh_kss_build_owned": (C.c_int, [vp, vp, GP, C.POINTER(SpssView), i32, C.POINTER(i32), C.POINTER(i32), i32,
                                          C.c_int, i32, C.POINTER(vp)]),
        "ksh_kss_comm_stats": (C.c_int, [vp, C.POINTER(i64)]),
        "ksh_comm_ranks_seen": (C.c_int, [vp, C.POINTER(i32)]),
        "ksh_kss_encode_counts": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "ksh_kss_weighed_counts": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "ksh_kss_phase_seconds": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "ksh_kss_destroy": (C.c_int, [vp]),
        "ksh_kss_size": (C.c_int, [vp, C.POINTER(i32)]),
        "ksh_kss_node": (C.c_int, [vp, i32, C.POINTER(SpssView), SP, C.POINTER(i64)]),
        "ksh_kss_children": (C.c_int, [vp, i32, C.POINTER(C.POINTER(i32)), C.POINTER(i32)]),
        "ksh_kss_meta": (C.c_char_p, [vp]),
        "ksh_kss_trace": (C.c_int, [vp, C.POINTER(i64), C.POINTER(C.POINTER(i64)), C.POINTER(i64),
                                    C.POINTER(C.POINTER(i64)), C.POINTER(C.POINTER(C.c_float))]),
        "ksh_kss_initial_weights": (C.c_int, [vp, C.POINTER(C.POINTER(i64)), C.POINTER(i64)]),
        "ksh_kss_stats": (C.c_int, [vp, C.POINTER(i64)]),
        "ksh_kss_get": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]),
        "ksh_kss_index_from_kss": (C.c_int, [vp, C.POINTER(vp)]),
        "ksh_kss_index_create": (C.c_int, [vp, GP, C.POINTER(SpssView), i32, C.POINTER(i64), C.POINTER(i32), C.c_int,
                                           C.POINTER(vp)]),
        "ksh_kss_index_query": (C.c_int, [vp, vp, i64, C.c_int, C.c_int, vp]),
        "ksh_kss_index_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]),
        "ksh_kss_index_routes": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "ksh_kss_index_destroy": (C.c_int, [vp]),
        "ksh_seq_hits": (C.c_int, [C.POINTER(SpssView), vp, C.c_int, C.c_int, i64, vp]),
        "ksh_kss_pair_counts": (C.c_int, [C.POINTER(i32), i32, vp, i64, vp, C.POINTER(i64)]),
        "ksh_kss_select_count": (C.c_int, [C.POINTER(Selection), vp, vp, C.POINTER(i64), C.POINTER(i64)]),
        "ksh_kss_select_keys": (C.c_int, [C.POINTER(Selection), vp, vp, i64, vp]),
        "ksh_kss_select_class_ids": (C.c_int, [C.POINTER(Selection), vp, C.POINTER(C.c_uint64), i64, vp, i64, vp, vp,
                                               C.POINTER(i64)]),
        "ksh_kss_color_classes": (C.c_int, [C.POINTER(i32), i32, vp, i64, C.POINTER(C.c_uint64), C.POINTER(i64),
                                            C.POINTER(i64)]),
        "ksh_seq_class_runs": (C.c_int, [C.POINTER(SpssView), vp, C.POINTER(SeqPaint), i64, vp, vp, vp, C.POINTER(i64),
                                         C.POINTER(i64)]),
        "ksh_spss_cut": (C.c_int, [C.POINTER(SpssView), vp, GP, vp, vp, i64, vp, vp, C.POINTER(i64)]),
        "ksh_spss_links": (C.c_int, [C.POINTER(SpssView), vp, GP, C.c_int, i64, vp, vp, C.POINTER(i64)]),
        "ksh_link_bubbles": (C.c_int, [C.POINTER(LinkGraph), vp, C.c_int32, i64, i64, vp, vp, vp, vp, C.POINTER(i64),
                                       C.POINTER(i64)]),
        "ksh_seq_locate": (C.c_int, [C.POINTER(LocateReq)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def exported_symbols():
    """Names declared in include/kmersets_hip.h (parsed from the header)."""
    import re

    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ksh_[a-z0-9_]+)\s*\(", text)))


def check(rc):
    if rc != KSH_OK:
        raise KshError(rc, lib().ksh_last_error().decode())


def geom(k, n_bucket_bits, key_bytes=None):
    """Device geometry of the reference's <K, N, KeyType>.  key_bytes: the reference's KeyType size (1, 2, 4
    or 8; None: the narrowest the key bits fit); device keys are 2, 4 or 8 bytes (uint8_t widens to 2)."""
    kb = 2 * k - n_bucket_bits
    if key_bytes is None:
        key_bytes = 2 if kb <= 16 else (4 if kb <= 32 else 8)
    return Geom(k, n_bucket_bits, 2 if key_bytes <= 2 else (4 if key_bytes <= 4 else 8), 0)


KEY_DTYPE = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def gfa_lines(strings, k, link_offsets, link_to, string_class=None):
    """GFA 1 text of a graph of strings, a list of lines without newlines: the header H\tVN:Z:1.0, a segment line
    S\t<r>\t<seq> per string (with \tCL:i:<class> when string_class is given) and a link line
    L\t<a>\t<+|->\t<b>\t<+|->\t<K-1>M for every link 2 a + (orientation -) -> 2 b + (orientation -) of
    link_offsets / link_to as Context.spss_links returns them (tensors, arrays or lists).  Every link is written: in
    canonical mode that is both twins, a -> b and the reverse complement of b -> the reverse complement of a."""
    def host(x):
        return np.asarray(x.cpu() if hasattr(x, "cpu") else x).reshape(-1)

    off, to = host(link_offsets).astype(np.int64), host(link_to).astype(np.int64)
    cls = None if string_class is None else host(string_class).astype(np.int64)
    n = len(strings)
    if off.size != 2 * n + 1 or (cls is not None and cls.size != n):
        raise ValueError("gfa_lines: %d strings need %d offsets (and %d classes)" % (n, 2 * n + 1, n))
    lines = ["H\tVN:Z:1.0"]
    for r, s in enumerate(strings):
        lines.append("S\t%d\t%s" % (r, s) + ("" if cls is None else "\tCL:i:%d" % cls[r]))
    overlap = "%dM" % (int(k) - 1)
    for v in range(2 * n):
        for w in to[off[v]:off[v + 1]]:
            lines.append("L\t%d\t%s\t%d\t%s\t%s" % (v >> 1, "-" if v & 1 else "+", int(w) >> 1,
                                                    "-" if int(w) & 1 else "+", overlap))
    return lines


def write_gfa(path, strings, k, link_offsets, link_to, string_class=None):
    """gfa_lines written to `path`, a newline behind every line.  Returns the number of lines."""
    lines = gfa_lines(strings, k, link_offsets, link_to, string_class)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


def _host_i64(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x).reshape(-1).astype(np.int64)


_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def bubble_alleles(strings, k, ends, arm_offsets, arm_strings):
    """The bubbles of Context.link_bubbles as text over the downloaded strings: one (v, w, allele_0, allele_1) per
    bubble.  An allele is its arm spelled: the oriented strings of the arm (2 s string s as written, 2 s + 1 its
    reverse complement) joined on their K - 1 overlaps, so it carries the K - 1 bases of the source's end in front
    and the K - 1 bases of the sink's start behind.  ends, arm_offsets, arm_strings: tensors, arrays or lists."""
    ends, off, arm = _host_i64(ends).reshape(-1, 2), _host_i64(arm_offsets), _host_i64(arm_strings)
    if off.size != 2 * len(ends) + 1:
        raise ValueError("bubble_alleles: %d bubbles need %d arm offsets" % (len(ends), 2 * len(ends) + 1))
    k = int(k)

    def spell(a):
        text = ""
        for x in arm[off[a]:off[a + 1]]:
            t = strings[int(x) >> 1]
            t = t.translate(_COMPLEMENT)[::-1] if int(x) & 1 else t
            text = t if not text else text + t[k - 1:]
        return text

    return [(int(v), int(w), spell(2 * b), spell(2 * b + 1)) for b, (v, w) in enumerate(ends)]


def bubble_lines(strings, k, ends, arm_offsets, arm_strings, arm_rows=None, n_cols=None):
    """One tab-separated line per bubble, without newlines: source, sink, allele_0, allele_1, the carriers of arm 0,
    the carriers of arm 1.  Source and sink are oriented strings; the alleles are bubble_alleles; the carriers of an
    arm are the comma-separated column positions whose bit is set in its row of arm_rows (uint64[2 nb, 2]; below
    n_cols if given), '.' for none -- also without arm_rows."""
    rows = None
    if arm_rows is not None:
        rows = np.asarray(arm_rows.cpu() if hasattr(arm_rows, "cpu") else arm_rows).reshape(-1, 2).astype(np.uint64)
    lines = []
    for b, (v, w, a0, a1) in enumerate(bubble_alleles(strings, k, ends, arm_offsets, arm_strings)):
        carriers = []
        for a in (2 * b, 2 * b + 1):
            bits = 0 if rows is None else int(rows[a, 0]) | int(rows[a, 1]) << 64
            cols = [str(c) for c in range(128 if n_cols is None else int(n_cols)) if bits >> c & 1]
            carriers.append(",".join(cols) if cols else ".")
        lines.append("%d\t%d\t%s\t%s\t%s\t%s" % (v, w, a0, a1, carriers[0], carriers[1]))
    return lines


def write_bubbles(path, strings, k, ends, arm_offsets, arm_strings, arm_rows=None, n_cols=None):
    """bubble_lines written to `path`, a newline behind every line.  Returns the number of lines."""
    lines = bubble_lines(strings, k, ends, arm_offsets, arm_strings, arm_rows, n_cols)
    with open(path, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    return len(lines)


UNPLACED_REASONS = ("anchor", "apart", "order", "off")


def place_bubbles(strings, k, ends, arm_offsets, arm_strings, where, count, ref_strings, arm_rows=None, n_cols=None):
    """The bubbles of Context.link_bubbles placed on a reference: one dict per bubble, in the bubbles' order.  where
    and count are Context.seq_locate of the graph's strings in the reference, ref_strings the reference's sequences as
    text.  A placed bubble is {"v", "w", "seq", "pos", "ref", "alt", "gt"}: sequence number, 1-based POS, the two
    trimmed alleles and, with arm_rows, one genotype per column below n_cols ("0" the column carries the REF arm only,
    "1" the ALT arm only, "0/1" both, "." neither), else None.  An unplaced one is {"v", "w", "unplaced": reason}:
      anchor  the exit end of v (end v ^ 1) or the entry end of w (end w) occurs in the reference not exactly once;
      apart   the two anchors lie in different sequences or on different strands;
      order   the sink's anchor does not lie behind the source's (after taking the twin on strand 1);
      off     neither allele spells the reference between the anchors.
    The reference text of the site is bases [p_a + 1, p_b + K - 1) of the sequence, p_a and p_b the positions of the
    two anchors; the arm that equals it is REF.  Common trailing bases are trimmed first, then common leading ones,
    each while both alleles are longer than one base; there is no left-alignment beyond the arms."""
    k = int(k)
    where, count = _host_i64(where), _host_i64(count)
    rows = None
    if arm_rows is not None:
        rows = np.asarray(arm_rows.cpu() if hasattr(arm_rows, "cpu") else arm_rows).reshape(-1, 2).astype(np.uint64)
    pstart = np.concatenate([[0], np.cumsum([len(t) - k + 1 for t in ref_strings])]).astype(np.int64)
    out = []
    for b, (v, w, a0, a1) in enumerate(bubble_alleles(strings, k, ends, arm_offsets, arm_strings)):
        entry = {"v": v, "w": w}
        out.append(entry)
        ev, ew = v ^ 1, w
        if count[ev] != 1 or count[ew] != 1:
            entry["unplaced"] = "anchor"
            continue
        g_v, s_v = int(where[ev]) >> 1, (int(where[ev]) & 1) ^ (v & 1)
        g_w, s_w = int(where[ew]) >> 1, (int(where[ew]) & 1) ^ (w & 1)
        r = int(np.searchsorted(pstart, g_v, side="right")) - 1
        if r != int(np.searchsorted(pstart, g_w, side="right")) - 1 or s_v != s_w:
            entry["unplaced"] = "apart"
            continue
        alleles = [a0, a1]
        if s_v:
            g_v, g_w = g_w, g_v
            alleles = [a.translate(_COMPLEMENT)[::-1] for a in alleles]
        if g_w <= g_v:
            entry["unplaced"] = "order"
            continue
        start, stop = g_v - int(pstart[r]) + 1, g_w - int(pstart[r]) + k - 1
        site = ref_strings[r][start:stop]
        if site not in alleles:
            entry["unplaced"] = "off"
            continue
        ref_arm = alleles.index(site)
        ref, alt = alleles[ref_arm], alleles[1 - ref_arm]
        while len(ref) > 1 and len(alt) > 1 and ref[-1] == alt[-1]:
            ref, alt = ref[:-1], alt[:-1]
        while len(ref) > 1 and len(alt) > 1 and ref[0] == alt[0]:
            ref, alt, start = ref[1:], alt[1:], start + 1
        gt = None
        if rows is not None:
            bits = [int(rows[2 * b + a, 0]) | int(rows[2 * b + a, 1]) << 64 for a in (ref_arm, 1 - ref_arm)]
            gt = [(".", "0", "1", "0/1")[(bits[0] >> c & 1) | (bits[1] >> c & 1) << 1]
                  for c in range(128 if n_cols is None else int(n_cols))]
        entry.update(seq=r, pos=start + 1, ref=ref, alt=alt, gt=gt)
    return out


def vcf_lines(records, ref_names, ref_lengths, sample_names=None):
    """VCF 4.2 text of the placed bubbles among `records` (place_bubbles), a list of lines without newlines, and the
    counts {"placed", "anchor", "apart", "order", "off"}: the header (fileformat, a contig line per reference
    sequence, the INFO line of BUB, with genotypes the FORMAT line of GT), the column line, and the records sorted
    by (sequence, POS, REF, ALT) with ID, QUAL and FILTER '.', BUB=<v>,<w> in INFO and, when the records carry
    genotypes, a GT column per sample (sample_names, by default S0, S1, ...).  Unplaced bubbles are only counted."""
    counts = dict.fromkeys(("placed",) + UNPLACED_REASONS, 0)
    placed = []
    for rec in records:
        counts[rec.get("unplaced", "placed")] += 1
        if "unplaced" not in rec:
            placed.append(rec)
    with_gt = bool(placed) and all(rec["gt"] is not None for rec in placed)
    lines = ["##fileformat=VCFv4.2"]
    lines += ["##contig=<ID=%s,length=%d>" % (name, int(n)) for name, n in zip(ref_names, ref_lengths)]
    lines.append('##INFO=<ID=BUB,Number=2,Type=Integer,Description="Source and sink of the bubble, oriented strings '
                 'of the graph">')
    cols = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"]
    if with_gt:
        lines.append('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">')
        n_samples = len(placed[0]["gt"])
        names = list(sample_names) if sample_names is not None else ["S%d" % c for c in range(n_samples)]
        if len(names) != n_samples:
            raise ValueError("vcf_lines: %d sample names for %d genotype columns" % (len(names), n_samples))
        cols += ["FORMAT"] + names
    lines.append("\t".join(cols))
    for rec in sorted(placed, key=lambda r: (r["seq"], r["pos"], r["ref"], r["alt"])):
        fields = [ref_names[rec["seq"]], str(rec["pos"]), ".", rec["ref"], rec["alt"], ".", ".",
                  "BUB=%d,%d" % (rec["v"], rec["w"])]
        if with_gt:
            fields += ["GT"] + list(rec["gt"])
        lines.append("\t".join(fields))
    return lines, counts


def write_vcf(path, records, ref_names, ref_lengths, sample_names=None):
    """vcf_lines written to `path`, a newline behind every line.  Returns the counts."""
    lines, counts = vcf_lines(records, ref_names, ref_lengths, sample_names)
    with open(path, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    return counts


class DeviceSet:
    """A k-mer set resident in HBM: offsets int64[2^N+1] + sorted keys (u32/u64 bytes)."""

    def __init__(self, g, offsets, keys_bytes, n_keys):
        self.g, self.offsets, self.keys, self.n_keys = g, offsets, keys_bytes, int(n_keys)

    @classmethod
    def carved(cls, g, off_rows, row, key_pool, byte_start, byte_len):
        """A set whose offsets are row `row` of off_rows and whose keys are a byte range of
        key_pool; the tensor slices are only made when somebody asks for them (a batch of pair
        results carves dozens of these per call)."""
        self = cls.__new__(cls)
        self.g, self.n_keys = g, 0
        self._carve = (off_rows, row, key_pool, byte_start, byte_len)
        self._ptrs = (off_rows.data_ptr() + row * off_rows.shape[1] * 8, key_pool.data_ptr() + byte_start)
        return self

    def __getattr__(self, name):
        # only reached for attributes that are not set: the lazily sliced tensors of carved()
        if name in ("offsets", "keys") and "_carve" in self.__dict__:
            off_rows, row, key_pool, byte_start, byte_len = self._carve
            self.offsets = off_rows[row]
            self.keys = key_pool[byte_start:byte_start + byte_len]
            return self.__dict__[name]
        raise AttributeError(name)

    def pointers(self):
        p = self.__dict__.get("_ptrs")
        return p if p is not None else (self.offsets.data_ptr(), self.keys.data_ptr())

    @classmethod
    def from_numpy(cls, g, offsets, keys, device):
        import torch

        kdt = KEY_DTYPE[g.key_bytes]
        keys = np.ascontiguousarray(keys, dtype=kdt)
        off_t = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(device)
        raw = torch.from_numpy(keys.view(np.uint8).copy()) if keys.size else torch.zeros(0, dtype=torch.uint8)
        key_t = torch.empty(max(raw.numel(), 16), dtype=torch.uint8, device=device)
        key_t[: raw.numel()] = raw.to(device)
        return cls(g, off_t, key_t, keys.size)

    @classmethod
    def from_kmers(cls, g, kmers, device):
        from . import synth

        offsets, keys = synth.to_bucketed(kmers, g.k, g.n_bucket_bits, g.key_bytes)
        return cls.from_numpy(g, offsets, keys, device)

    @classmethod
    def empty_like_offsets(cls, g, n_keys, device):
        import torch

        off = torch.empty((1 << g.n_bucket_bits) + 1, dtype=torch.int64, device=device)
        keys = torch.empty(max(int(n_keys) * g.key_bytes, 16), dtype=torch.uint8, device=device)
        return cls(g, off, keys, n_keys)

    def view(self):
        po, pk = self.pointers()
        return SetView(po, pk, self.n_keys)

    def to_numpy(self):
        kdt = KEY_DTYPE[self.g.key_bytes]
        keys = self.keys[: self.n_keys * self.g.key_bytes].cpu().numpy().view(kdt)
        return self.offsets.cpu().numpy(), keys

    def kmers(self):
        from . import synth

        off, keys = self.to_numpy()
        return synth.from_bucketed(off, keys, self.g.k, self.g.n_bucket_bits)


class DeviceSpss:
    """KmerSetCompact on device: 2-bit bases in 64-bit words + (len - K) per string."""

    def __init__(self, g, words, lens, n_strings, n_bases):
        self.g, self.words, self.lens = g, words, lens
        self.n_strings, self.n_bases = int(n_strings), int(n_bases)

    @classmethod
    def from_strings(cls, g, strings, device):
        import torch
        from . import synth

        words, lens = synth.pack_strings(strings, g.k)
        w = torch.from_numpy(words.view(np.int64).copy()).to(device)
        ln = torch.from_numpy(lens.view(np.int32).copy()).to(device)
        if w.numel() == 0:
            w = torch.zeros(1, dtype=torch.int64, device=device)
        if ln.numel() == 0:
            ln = torch.zeros(1, dtype=torch.int32, device=device)
        return cls(g, w, ln, len(strings), int(sum(len(x) for x in strings)))

    def view(self):
        return SpssView(self.words.data_ptr(), self.lens.data_ptr(), self.n_strings, self.n_bases)

    def to_strings(self):
        from . import synth

        n_words = (self.n_bases + 31) // 32
        words = self.words[:n_words].cpu().numpy().view(np.uint64)
        lens = self.lens[: self.n_strings].cpu().numpy().view(np.uint32)
        return synth.unpack_strings(words, lens, self.g.k)

    def weight(self):
        return self.n_bases


class Pending:
    """What a plan-only wrapper of Context returns and the matching write-only wrapper takes: the plan's arguments
    (kept alive) and the sizes it returned.  The plan itself lives inside the context (include/kmersets_hip.h,
    "Plans")."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


class BatchResult:
    """Results of Context.pair_algebra_batch: indexable / iterable as [(A & B, A \\ B, B \\ A), ...];
    the DeviceSet objects (slices of the two batch-wide allocations) are made on first access;
    `totals` is the list [pair][|A&B|, |A\\B|, |B\\A|]."""

    def __init__(self, g, off_rows, key_pool, starts, byte_caps, totals):
        self.g, self.off_rows, self.key_pool, self.starts, self.byte_caps = g, off_rows, key_pool, starts, byte_caps
        self.totals = totals
        self._made = {}

    def __len__(self):
        return len(self.totals)

    def __getitem__(self, idx):
        if idx < 0:
            idx += len(self)
        if idx not in self._made:
            trio = []
            for r in range(3):
                s_ = DeviceSet.carved(self.g, self.off_rows, 3 * idx + r, self.key_pool,
                                      self.starts[3 * idx + r], self.byte_caps[3 * idx + r])
                s_.n_keys = self.totals[idx][r]
                trio.append(s_)
            self._made[idx] = trio
        return self._made[idx]

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class Context:
    """ksh_ctx on one GPU; its stream becomes torch's current stream on that device."""

    def __init__(self, device_index=0):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the k-mer set hot path has no CPU fallback")
        self.device = torch.device("cuda", device_index)
        torch.cuda.set_device(self.device)
        # One stream for everything: the library's kernels and torch's copies/allocations
        # are ordered against each other only if they share a stream (torch's default
        # stream has handle 0, which the C ABI reads as "make me a stream").
        self.stream = torch.cuda.Stream(device=self.device)
        torch.cuda.set_stream(self.stream)
        h = C.c_void_p()
        check(lib().ksh_ctx_create(device_index, C.c_void_p(self.stream.cuda_stream), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().ksh_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the module globals may already be gone: the process's exit
        # releases the device memory then
        if lib is not None and _lib is not None:
            self.close()

    def sync(self):
        check(lib().ksh_ctx_sync(self.h))

    def enable_timing(self, on=True):
        check(lib().ksh_ctx_enable_timing(self.h, int(on)))

    def timing_reset(self):
        check(lib().ksh_ctx_timing_reset(self.h))

    def timing_read(self, kind):
        """(summed ms, launches) of the timed kernel kind since the last reset."""
        ms, n = C.c_float(), C.c_int64()
        check(lib().ksh_ctx_timing_read(self.h, kind, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_units(self, kind):
        """k-mers (keys) covered by the timed launches of a kind since the last reset."""
        n = C.c_int64()
        check(lib().ksh_ctx_timing_units(self.h, kind, C.byref(n)))
        return n.value

    def timing_wall(self, kind):
        """ms during which at least one timed launch of the kind was running on any lane (union of the spans)."""
        ms = C.c_float()
        check(lib().ksh_ctx_timing_wall(self.h, kind, C.byref(ms)))
        return ms.value

    def mem_stats(self, reset_peak=False):
        """Device bytes behind the context: pooled buffers in use, their peak, cached, own scratch, lanes' total."""
        st = (C.c_int64 * 6)()
        check(lib().ksh_ctx_mem_stats(self.h, st, int(bool(reset_peak))))
        return {"pool_live": st[0], "pool_peak": st[1], "pool_cached": st[2], "scratch": st[3], "lanes": st[4],
                "n_lanes": st[5]}

    def set_lanes(self, n):
        """Independent jobs of one call (a check's encodes, the inputs' decodes) on up to n streams at once; 1: one
        stream, 0: the default (KSH_LANES, else 4)."""
        check(lib().ksh_ctx_set_lanes(self.h, int(n)))

    # test hooks (exported, not in the public header) ---------------------------------------
    def debug_scratch_fill(self, byte):
        """Scratch whose contents are undefined by contract is set to `byte` (0..255) before it is handed out, on this
        context and its lanes; None or -1: off.  The counters of debug_scratch_fill_stats restart."""
        fn = lib().ksh_debug_set_scratch_fill
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        check(fn(self.h, -1 if byte is None else int(byte)))

    def debug_scratch_fill_stats(self):
        """(fills, bytes filled) since the fill value was last set, the lanes' included."""
        fn = lib().ksh_debug_scratch_fill_stats
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
        st = (C.c_int64 * 2)()
        check(fn(self.h, st))
        return st[0], st[1]

    def debug_scan_epoch(self, set_to=None):
        """The epoch of the context's last chained scan (csrc/ksh_scan.h); set_to: the epoch it is set to first (the
        scan state stays as it is)."""
        fn = lib().ksh_debug_scan_epoch
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        now = C.c_int()
        check(fn(self.h, -1 if set_to is None else int(set_to), C.byref(now)))
        return now.value

    # KmerSet::Hash / Size -------------------------------------------------------
    def set_hash(self, s):
        out = C.c_uint64()
        v = s.view()
        check(lib().ksh_set_hash(self.h, C.byref(s.g), C.byref(v), C.byref(out)))
        return out.value

    # ParallelDisjointSet ----------------------------------------------------------------
    def dsu_components(self, n, xs, ys):
        """Unites the pairs (xs[i], ys[i]) over n nodes concurrently; returns Find(i) for every node."""
        import torch

        x = torch.from_numpy(np.ascontiguousarray(xs, dtype=np.int32)).to(self.device)
        y = torch.from_numpy(np.ascontiguousarray(ys, dtype=np.int32)).to(self.device)
        root = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        check(lib().ksh_dsu_components(self.h, n, x.data_ptr() if x.numel() else None,
                                       y.data_ptr() if y.numel() else None, x.numel(), root.data_ptr()))
        return root[:n].cpu().numpy()

    # KmerSet::Contains / Find -----------------------------------------------------------
    def set_contains(self, s, kmers):
        """bool array: which of the 2K-bit patterns `kmers` are in the set (one launch)."""
        import torch

        q = torch.from_numpy(np.ascontiguousarray(kmers, dtype=np.uint64).view(np.int64).copy()).to(self.device)
        out = torch.zeros(max(q.numel(), 1), dtype=torch.uint8, device=self.device)
        v = s.view()
        check(lib().ksh_set_contains(self.h, C.byref(s.g), C.byref(v), q.data_ptr(), q.numel(), out.data_ptr()))
        return out[: q.numel()].cpu().numpy().astype(bool)

    def set_kmers(self, s):
        """All k-mers of the set as uint64 bit patterns, ascending (expanded on the device)."""
        import torch

        out = torch.empty(max(s.n_keys, 1), dtype=torch.int64, device=self.device)
        v = s.view()
        check(lib().ksh_set_kmers(self.h, C.byref(s.g), C.byref(v), out.data_ptr()))
        return out[: s.n_keys].cpu().numpy().view(np.uint64)

    # Intersection / Sub -----------------------------------------------------------
    def pair_plan(self, a, b, out_i, out_amb, out_bma):
        totals = (C.c_int64 * 3)()
        va, vb = a.view(), b.view()
        check(lib().ksh_pair_plan(self.h, C.byref(a.g), C.byref(va), C.byref(vb),
                                  out_i.offsets.data_ptr(), out_amb.offsets.data_ptr(),
                                  out_bma.offsets.data_ptr(), totals))
        return [int(x) for x in totals]

    def pair_write(self, a, b, out_i, out_amb, out_bma, g=None):
        va, vb = a.view(), b.view()
        check(lib().ksh_pair_write(self.h, C.byref(a.g if g is None else g), C.byref(va), C.byref(vb),
                                   out_i.keys.data_ptr() if out_i is not None else None,
                                   out_amb.keys.data_ptr() if out_amb is not None else None,
                                   out_bma.keys.data_ptr() if out_bma is not None else None))

    def pair_algebra(self, a, b):
        """(A & B, A \\ B, B \\ A) as new DeviceSets (exact-size key buffers)."""
        import torch

        g = a.g
        outs = [DeviceSet.empty_like_offsets(g, 0, self.device) for _ in range(3)]
        totals = self.pair_plan(a, b, *outs)
        for o, n in zip(outs, totals):
            o.n_keys = n
            o.keys = torch.empty(max(n * g.key_bytes, 16), dtype=torch.uint8, device=self.device)
        self.pair_write(a, b, *outs)
        return outs

    # KmerSetCompact::Size / ToKmerSet ---------------------------------------------------
    def spss_size(self, sp):
        out = C.c_int64()
        v = sp.view()
        check(lib().ksh_spss_size(self.h, C.byref(sp.g), C.byref(v), C.byref(out)))
        return out.value

    def spss_decode_plan(self, sp, canonical=True):
        """ksh_spss_decode_plan alone: a Pending with the container, the flag, `out` (a DeviceSet whose offsets
        the plan filled, keys not yet allocated) and n_keys, the size of the key buffer the write needs."""
        out = DeviceSet.empty_like_offsets(sp.g, 0, self.device)
        n = C.c_int64()
        v = sp.view()
        check(lib().ksh_spss_decode_plan(self.h, C.byref(sp.g), C.byref(v), int(canonical),
                                         out.offsets.data_ptr(), C.byref(n)))
        return Pending(kind="decode", sp=sp, canonical=bool(canonical), out=out, n_keys=n.value)

    def _decode_keys(self, plan, keys):
        import torch

        if keys is None:
            keys = torch.empty(max(plan.n_keys * plan.sp.g.key_bytes, 16), dtype=torch.uint8, device=self.device)
        plan.out.keys = keys
        return keys

    def spss_decode_write(self, plan, keys=None, g=None, canonical=None, sp=None):
        """ksh_spss_decode_write on a Pending of spss_decode_plan (possibly one made on another Context).  keys: a
        uint8 tensor of at least n_keys * key_bytes bytes (allocated when None); g / canonical / sp replace the
        planned arguments (the library refuses a write whose arguments differ from the plan's)."""
        keys = self._decode_keys(plan, keys)
        g = plan.sp.g if g is None else g
        v = (plan.sp if sp is None else sp).view()
        n = C.c_int64()
        check(lib().ksh_spss_decode_write(self.h, C.byref(g), C.byref(v),
                                          int(plan.canonical if canonical is None else canonical),
                                          plan.out.offsets.data_ptr(), keys.data_ptr(), C.byref(n)))
        plan.out.n_keys = n.value
        return plan.out

    def kmer_count_write(self, plan, cutoff, keys=None, g=None, canonical=None):
        """ksh_kmer_count_write on a Pending of spss_decode_plan: (DeviceSet of the k-mers seen >= cutoff times,
        number of distinct k-mers below the cutoff)."""
        keys = self._decode_keys(plan, keys)
        g = plan.sp.g if g is None else g
        v = plan.sp.view()
        n, n_cut = C.c_int64(), C.c_int64()
        check(lib().ksh_kmer_count_write(self.h, C.byref(g), C.byref(v),
                                         int(plan.canonical if canonical is None else canonical), int(cutoff),
                                         plan.out.offsets.data_ptr(), keys.data_ptr(), C.byref(n), C.byref(n_cut)))
        plan.out.n_keys = n.value
        return plan.out, n_cut.value

    def spss_decode(self, sp, canonical=True):
        return self.spss_decode_write(self.spss_decode_plan(sp, canonical))

    # KmerCounter::FromFASTA / FromReads / ToKmerSet -------------------------------------------
    def fasta_plan(self, g, text):
        """ksh_fasta_plan alone: a Pending with n_strings (fragments) and n_bases."""
        n_frag, n_bases = C.c_int64(), C.c_int64()
        check(lib().ksh_fasta_plan(self.h, C.byref(g), text.data_ptr() if text.numel() else None,
                                   text.numel(), C.byref(n_frag), C.byref(n_bases)))
        return Pending(kind="fasta", g=g, text=text, n_strings=n_frag.value, n_bases=n_bases.value)

    def fasta_write(self, plan, words=None, lens=None, plain=False):
        text = plan.text.data_ptr() if plan.text.numel() else None
        return self._write_spss("ksh_fasta_write", plan, words, lens, text, plain, zero=True)

    def fasta_fragments(self, g, text):
        """uint8 tensor (device) holding FASTA text -> DeviceSpss of the reads' ACGT fragments
        of length >= K (what the counter counts k-mers of)."""
        return self.fasta_write(self.fasta_plan(g, text))

    def kmer_count(self, reads, cutoff, canonical=True):
        """(KmerSet of the k-mers seen >= cutoff times in the fragments, number of distinct
        k-mers below the cutoff)."""
        return self.kmer_count_write(self.spss_decode_plan(reads, canonical), cutoff)

    def _spss_buffers(self, plan, words, lens, zero=False):
        """The output buffers of a container-producing write, sized from the plan (int64 words, int32 lens)."""
        import torch

        make = torch.zeros if zero else torch.empty
        if words is None:
            words = make(max((plan.n_bases + 31) // 32, 1), dtype=torch.int64, device=self.device)
        if lens is None:
            lens = make(max(plan.n_strings, 1), dtype=torch.int32, device=self.device)
        return words, lens

    def _write_spss(self, name, plan, words, lens, d_input, plain, zero=False):
        """One of the four writes that name no input, on a Pending of its plan: the `_for` form, which states the
        plan it means (the planned sizes and input pointer), or with plain=True the three-argument form."""
        words, lens = self._spss_buffers(plan, words, lens, zero=zero)
        if plain:
            check(getattr(lib(), name)(self.h, words.data_ptr(), lens.data_ptr()))
        else:
            check(getattr(lib(), name + "_for")(self.h, words.data_ptr(), lens.data_ptr(), plan.n_strings,
                                                plan.n_bases, d_input))
        return DeviceSpss(plan.g, words, lens, plan.n_strings, plan.n_bases)

    # KmerSetCompact::Dump / Load text (one string per line) ------------------------------
    def spss_to_text(self, sp):
        """The bytes KmerSetCompact::Dump writes, as a uint8 tensor on the device."""
        import torch

        text = torch.empty(sp.n_bases + sp.n_strings, dtype=torch.uint8, device=self.device)
        v = sp.view()
        check(lib().ksh_spss_to_text(self.h, C.byref(sp.g), C.byref(v), text.data_ptr() if text.numel() else None))
        return text

    def spss_from_text_plan(self, g, text):
        """ksh_spss_from_text_plan alone: a Pending with n_strings and n_bases."""
        n_strings, n_bases = C.c_int64(), C.c_int64()
        check(lib().ksh_spss_from_text_plan(self.h, C.byref(g), text.data_ptr() if text.numel() else None,
                                            text.numel(), C.byref(n_strings), C.byref(n_bases)))
        return Pending(kind="from_text", g=g, text=text, n_strings=n_strings.value, n_bases=n_bases.value)

    def spss_from_text_write(self, plan, words=None, lens=None, plain=False):
        text = plan.text.data_ptr() if plan.text.numel() else None
        return self._write_spss("ksh_spss_from_text_write", plan, words, lens, text, plain)

    def spss_from_text(self, g, text):
        """uint8 tensor (device) holding lines over ACGT -> DeviceSpss."""
        return self.spss_from_text_write(self.spss_from_text_plan(g, text))

    # KmerSetCompact::FromKmerSet / GetUnitigsCanonical ---------------------------------------
    def spss_encode_plan(self, s, mode=0, canonical=True):
        """ksh_spss_encode_plan alone: a Pending with n_strings and n_bases."""
        ns, nbases = C.c_int64(), C.c_int64()
        v = s.view()
        check(lib().ksh_spss_encode_plan(self.h, C.byref(s.g), C.byref(v), int(canonical), mode,
                                         C.byref(ns), C.byref(nbases)))
        return Pending(kind="encode", g=s.g, set=s, n_strings=ns.value, n_bases=nbases.value)

    def spss_encode_write(self, plan, words=None, lens=None, plain=False):
        return self._write_spss("ksh_spss_encode_write", plan, words, lens, plan.set.pointers()[0], plain)

    def spss_encode_release(self):
        check(lib().ksh_spss_encode_release(self.h))

    def spss_encode(self, s, mode=0, canonical=True):
        """mode 0: SPSS (GetSPSSCanonical fast, or GetSPSS when canonical is False); mode 1: unitigs;
        mode 2: GetSPSSCanonical(fast = false).  Returns a DeviceSpss."""
        return self.spss_encode_write(self.spss_encode_plan(s, mode, canonical))

    def spss_cut(self, seqs, run_offsets, run_start):
        """ksh_spss_cut: the strings of `seqs` (a DeviceSpss) cut at the runs (run_offsets int64[n_strings + 1],
        run_start int32 or uint32 [n_runs], device tensors as KssIndex.class_runs returns them; n_runs is the size of
        run_start) into one string per run, K - 1 bases repeated at every cut: the same k-mers in the same order.
        Returns a DeviceSpss of n_runs strings."""
        import torch

        with torch.cuda.stream(self.stream):
            n, n_runs = seqs.n_strings, int(run_start.numel())
            off = run_offsets.contiguous()
            if off.dtype != torch.int64 or off.numel() != n + 1:
                raise ValueError("run_offsets: int64[n_strings + 1] = int64[%d] wanted, %s[%d] given"
                                 % (n + 1, off.dtype, off.numel()))
            start = run_start.contiguous()
            if start.element_size() != 4 or start.is_floating_point():
                raise ValueError("run_start: int32 or uint32 wanted, %s given" % start.dtype)
            n_out = seqs.n_bases + (n_runs - n) * (seqs.g.k - 1)  # (the closed form: no plan call)
            words = torch.empty(max((max(n_out, 0) + 31) // 32, 1), dtype=torch.int64, device=self.device)
            lens = torch.empty(max(n_runs, 1), dtype=torch.int32, device=self.device)
            view, got = seqs.view(), C.c_int64()
            check(lib().ksh_spss_cut(C.byref(view), self.h, C.byref(seqs.g), off.data_ptr(),
                                     start.data_ptr() if n_runs else None, n_runs, words.data_ptr(), lens.data_ptr(),
                                     C.byref(got)))
            assert got.value == n_out
            return DeviceSpss(seqs.g, words, lens, n_runs, n_out)

    def spss_links_raw(self, seqs, canonical, capacity, offsets=None, link_to=None):
        """ksh_spss_links, one call: (rc, n_links).  offsets, link_to: device int64 tensors or None.  rc is KSH_OK or
        KSH_FAILED_PRECONDITION (too small a capacity: the message is ksh_last_error); anything else is raised."""
        import torch

        with torch.cuda.stream(self.stream):
            view, n = seqs.view(), C.c_int64(-1)
            rc = lib().ksh_spss_links(C.byref(view), self.h, C.byref(seqs.g), int(bool(canonical)), int(capacity),
                                      offsets.data_ptr() if offsets is not None else None,
                                      link_to.data_ptr() if link_to is not None else None, C.byref(n))
            if rc not in (KSH_OK, KSH_FAILED_PRECONDITION):
                check(rc)
            return rc, n.value

    def spss_links(self, seqs, canonical=True):
        """ksh_spss_links: the links between the strings of `seqs` (a DeviceSpss), the edges of the graph whose nodes
        the strings are.  The oriented string v = 2 s + o is string s as written (o = 0) or reverse-complemented
        (o = 1); v -> w is a link when the last k-mer of v moved on by one base is the first k-mer of w (a k-mer
        followed by itself, or with `canonical` by its reverse complement, is none).  Returns (link_offsets, link_to),
        device int64 tensors [2 n + 1] and [n_links]: the links of v are link_to[link_offsets[v]:link_offsets[v + 1]],
        ascending by the appended base.  canonical False: only the rows 2 s have links.  Only string ends are looked
        at; on unitigs or cuts of them (spss_encode mode 1, spss_cut) that is the whole graph.  One call counts, a
        second one fills."""
        import torch

        with torch.cuda.stream(self.stream):
            off = torch.zeros(2 * seqs.n_strings + 1, dtype=torch.int64, device=self.device)
        rc, n_links = self.spss_links_raw(seqs, canonical, 0, off)
        check(rc)
        with torch.cuda.stream(self.stream):
            link_to = torch.empty(max(n_links, 1), dtype=torch.int64, device=self.device)
        if n_links:
            rc, again = self.spss_links_raw(seqs, canonical, n_links, off, link_to)
            check(rc)
            assert again == n_links
        return off, link_to[:n_links]

    def link_bubbles_raw(self, link_offsets, link_to, max_arm, capacity, arm_capacity, ends=None, arm_offsets=None,
                         arm_strings=None, arm_rows=None, string_class=None, rows=None, n_strings=None, n_links=None):
        """ksh_link_bubbles, one call: (rc, n_bubbles, n_arm_strings).  link_offsets, link_to, string_class and the
        four outputs: device tensors or None; rows: a host class table or None.  n_strings, n_links: what the graph
        claims, by default what the tensors hold.  rc is KSH_OK or KSH_FAILED_PRECONDITION (too small a capacity: the
        message is ksh_last_error); anything else is raised."""
        import torch

        with torch.cuda.stream(self.stream):
            table = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
            n = (link_offsets.numel() - 1) // 2 if n_strings is None else int(n_strings)
            links = (0 if link_to is None else link_to.numel()) if n_links is None else int(n_links)
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            graph = LinkGraph(C.sizeof(LinkGraph), n, ptr(link_offsets), ptr(link_to), links, ptr(string_class),
                              None if table is None else table.ctypes.data_as(C.POINTER(C.c_uint64)),
                              0 if table is None else table.size // 2)
            nb, na = C.c_int64(-1), C.c_int64(-1)
            rc = lib().ksh_link_bubbles(C.byref(graph), self.h, int(max_arm), int(capacity), int(arm_capacity),
                                        ptr(ends), ptr(arm_offsets), ptr(arm_strings), ptr(arm_rows), C.byref(nb),
                                        C.byref(na))
            del table
            if rc not in (KSH_OK, KSH_FAILED_PRECONDITION):
                check(rc)
            return rc, nb.value, na.value

    def link_bubbles(self, link_offsets, link_to, max_arm=8, string_class=None, rows=None):
        """ksh_link_bubbles: the bubbles of the link graph that spss_links returns in canonical mode (device int64
        tensors [2 n + 1] and [n_links]).  A bubble is a source v with two links, two arms of at most max_arm strings
        each -- every arm string has one link in and one out -- and the sink w where both arms end; it is reported
        once, as the twin with v <= w ^ 1, ascending by v.  Returns (ends int64[nb, 2], arm_offsets int64[2 nb + 1],
        arm_strings int64[...], arm_rows uint64[2 nb, 2] or None), device tensors: arm i of bubble b is
        arm_strings[arm_offsets[2 b + i]:arm_offsets[2 b + i + 1]], oriented strings in walk order, arm 0 the arm of
        the lower base.  With string_class (device int32[n]) and rows (a class table as color_classes returns it)
        arm_rows holds the carriers of every arm: the AND of the rows of its strings' classes, the sets that hold
        every k-mer of the allele; a set that holds only part of an arm is not a carrier.  One call counts, a second
        one fills."""
        import torch

        kw = dict(string_class=string_class, rows=rows)
        rc, nb, na = self.link_bubbles_raw(link_offsets, link_to, max_arm, 0, 0, **kw)
        check(rc)
        with torch.cuda.stream(self.stream):
            ends = torch.empty(2 * max(nb, 1), dtype=torch.int64, device=self.device)
            arm_off = torch.zeros(2 * max(nb, 1) + 1, dtype=torch.int64, device=self.device)
            arm = torch.empty(max(na, 1), dtype=torch.int64, device=self.device)
            arm_rows = None if rows is None else torch.empty(4 * max(nb, 1), dtype=torch.uint64, device=self.device)
        if nb:
            rc, again, again_arm = self.link_bubbles_raw(link_offsets, link_to, max_arm, nb, na, ends, arm_off, arm,
                                                         arm_rows, **kw)
            check(rc)
            assert (again, again_arm) == (nb, na)
        return (ends[:2 * nb].reshape(nb, 2), arm_off[:2 * nb + 1], arm[:na],
                None if arm_rows is None else arm_rows[:4 * nb].reshape(2 * nb, 2))

    def seq_locate_raw(self, strings, reference, canonical, where=None, count=None, g=None, struct_size=None,
                       want_located=True):
        """ksh_seq_locate, one call: (rc, n_located).  strings, reference: a DeviceSpss, an SpssView or None; where
        (int64) and count (uint32 or int32): device tensors or None.  g: the geometry, by default that of `strings`.
        rc is the return code, whatever it is: the message is ksh_last_error."""
        import torch

        with torch.cuda.stream(self.stream):
            view = lambda x: x.view() if isinstance(x, DeviceSpss) else x  # noqa: E731
            sv, rv = view(strings), view(reference)
            g = strings.g if g is None else g
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            got = C.c_int64(-1)
            req = LocateReq(C.sizeof(LocateReq) if struct_size is None else int(struct_size), self.h,
                            None if g is None else C.pointer(g), None if sv is None else C.pointer(sv),
                            None if rv is None else C.pointer(rv), int(bool(canonical)), ptr(where), ptr(count),
                            C.pointer(got) if want_located else None)
            rc = lib().ksh_seq_locate(C.byref(req))
            return rc, got.value

    def seq_locate(self, strings, reference, canonical=True):
        """ksh_seq_locate: where the ends of `strings` occur in `reference` (both a DeviceSpss).  End 2 s is the first
        k-mer of string s as written, end 2 s + 1 its last.  Returns (where, count), device tensors int64[2 n] and
        uint32[2 n]: count[e] is the number of k-mer positions of the reference that hold the end's k-mer (with
        `canonical`, or its reverse complement), where[e] is (g << 1) | strand of the one with the smallest global
        position g, strand 1 meaning that the reference reads the reverse complement, or -1.  Global positions number
        the k-mer positions of all reference sequences in one line: sequence r owns len(r) - K + 1 of them, in the
        container's order (place_bubbles turns them back)."""
        import torch

        n = strings.n_strings
        with torch.cuda.stream(self.stream):
            where = torch.empty(2 * n, dtype=torch.int64, device=self.device)
            count = torch.empty(2 * n, dtype=torch.uint32, device=self.device)
        rc, _ = self.seq_locate_raw(strings, reference, canonical, where, count)
        check(rc)
        return where, count

    def spss_encode_stats(self):
        st = (C.c_int64 * 4)()
        check(lib().ksh_spss_encode_stats(self.h, st))
        return {"unitigs": st[0], "rounds": st[1], "strings": st[2], "bases": st[3]}

    # GetSPSSCanonical / GetSPSS from caller-supplied unitigs -----------------------------------
    def spss_cover_plan(self, unitigs, canonical=True, fast=True):
        """ksh_spss_cover_plan alone: a Pending with n_strings and n_bases (the input must stay alive until the
        write)."""
        ns, nbases = C.c_int64(), C.c_int64()
        v = unitigs.view()
        check(lib().ksh_spss_cover_plan(self.h, C.byref(unitigs.g), C.byref(v), int(canonical), int(fast),
                                        C.byref(ns), C.byref(nbases)))
        return Pending(kind="cover", g=unitigs.g, unitigs=unitigs, n_strings=ns.value, n_bases=nbases.value)

    def spss_cover_write(self, plan, words=None, lens=None, plain=False):
        return self._write_spss("ksh_spss_cover_write", plan, words, lens, plan.unitigs.words.data_ptr(), plain)

    def spss_cover_release(self):
        check(lib().ksh_spss_cover_release(self.h))

    def spss_cover(self, unitigs, canonical=True, fast=True):
        """The path cover of a DeviceSpss whose strings are unitigs (GetSPSSCanonical(unitigs, prefixes, suffixes,
        fast), or GetSPSS(unitigs, prefixes) when canonical is False).  Returns a DeviceSpss; the input must
        meet the preconditions of ksh_spss_cover_plan (include/kmersets_hip.h), else KshError."""
        return self.spss_cover_write(self.spss_cover_plan(unitigs, canonical, fast))

    def spss_cover_stats(self):
        st = (C.c_int64 * 4)()
        check(lib().ksh_spss_cover_stats(self.h, st))
        return {"unitigs": st[0], "rounds": st[1], "strings": st[2], "bases": st[3]}

    ROUTES = ("probe_staged", "rc_1024", "rc_512", "rc_256", "rc_64", "rc_batched", "scatter_two_level",
              "fwd_staged", "rank_one_launch", "heads_one_launch", "jump_two_level", "rank_stamped", "emit_logs",
              "long_stretches", "match_more_rounds", "fwd_targets", "rc1_streamed", "rc_marks_groups",
              "tgt_parts")

    def spss_encode_routes(self):
        """The kernel variants the last encode plan ran (KSH_ROUTE_* of include/kmersets_hip.h), as a set of names."""
        r = C.c_int64()
        check(lib().ksh_spss_encode_routes(self.h, C.byref(r)))
        return {name for bit, name in enumerate(self.ROUTES) if r.value >> bit & 1}

    def pair_algebra_onepass(self, a, b):
        """(A & B, A \\ B, B \\ A) by ksh_pair_algebra (count + write passes enqueued back to
        back); key buffers are allocated at their upper bounds before the sizes are known."""
        import torch

        g = a.g
        caps = (min(a.n_keys, b.n_keys), a.n_keys, b.n_keys)
        outs = []
        for cap in caps:
            o = DeviceSet.empty_like_offsets(g, 0, self.device)
            o.keys = torch.empty(max(cap * g.key_bytes, 16), dtype=torch.uint8, device=self.device)
            outs.append(o)
        totals = (C.c_int64 * 3)()
        va, vb = a.view(), b.view()
        check(lib().ksh_pair_algebra(self.h, C.byref(g), C.byref(va), C.byref(vb),
                                     outs[0].offsets.data_ptr(), outs[1].offsets.data_ptr(),
                                     outs[2].offsets.data_ptr(), outs[0].keys.data_ptr(),
                                     outs[1].keys.data_ptr(), outs[2].keys.data_ptr(), totals))
        for o, n in zip(outs, totals):
            o.n_keys = int(n)
        return outs

    def svb_encode(self, values):
        """StreamVByte-0124 bytes of a uint32 array (device round trip)."""
        import torch

        v = np.ascontiguousarray(values, dtype=np.uint32)
        d_in = torch.from_numpy(v.view(np.int32).copy()).to(self.device) if v.size else torch.zeros(1, dtype=torch.int32, device=self.device)
        cap = (v.size + 3) // 4 + 4 * v.size
        d_out = torch.empty(max(cap, 16), dtype=torch.uint8, device=self.device)
        n = C.c_int64()
        check(lib().ksh_svb_encode_0124(self.h, d_in.data_ptr(), v.size, d_out.data_ptr(), C.byref(n)))
        return d_out[: n.value].cpu().numpy()

    def svb_decode(self, data, n):
        import torch

        d = np.ascontiguousarray(data, dtype=np.uint8)
        d_in = torch.from_numpy(d.copy()).to(self.device) if d.size else torch.zeros(16, dtype=torch.uint8, device=self.device)
        d_out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        used = C.c_int64()
        check(lib().ksh_svb_decode_0124(self.h, d_in.data_ptr(), n, d_out.data_ptr(), C.byref(used)))
        return d_out[:n].cpu().numpy().view(np.uint32), used.value

    def pair_algebra_batch(self, pairs):
        """[(A, B), ...] -> [(A & B, A \\ B, B \\ A), ...]: every pair of the batch tiled together, one
        count launch, one write launch and one stream synchronisation for all sizes
        (ksh_pair_algebra_batch).  The result behaves like that list; `.totals` is the list
        [pair][|A&B|, |A\\B|, |B\\A|] for callers that only need the sizes."""
        import torch

        g = pairs[0][0].g
        kb = g.key_bytes
        n = len(pairs)
        # The job records as one int64 table with PairJob's layout (15 eight-byte fields):
        # a.{offsets, keys, n}, b.{offsets, keys, n}, 3 offset pointers, 3 key pointers, 3 totals.
        # Built with plain integers and converted once: a handful of pairs is far below the size
        # where numpy's per-call cost pays, and this runs once per merge step.
        assert C.sizeof(PairJob) == 15 * 8
        nb1 = (1 << g.n_bucket_bits) + 1
        byte_caps, starts = [], [0]
        for a, b in pairs:
            for cap in (min(a.n_keys, b.n_keys), a.n_keys, b.n_keys):
                nbytes = max(cap * kb, 16)
                byte_caps.append(nbytes)
                starts.append(starts[-1] + ((nbytes + 255) & ~255))       # bytes reserved per result
        # one offsets block and one key pool for the whole batch, carved by pointer arithmetic
        off_rows = torch.empty((3 * n, nb1), dtype=torch.int64, device=self.device)
        key_pool = torch.empty(starts[-1], dtype=torch.uint8, device=self.device)
        off0, key0 = off_rows.data_ptr(), key_pool.data_ptr()
        rows = []
        for idx, (a, b) in enumerate(pairs):
            pa, pb = a.pointers(), b.pointers()
            r = 3 * idx
            rows.append((pa[0], pa[1], a.n_keys, pb[0], pb[1], b.n_keys,
                         off0 + 8 * nb1 * r, off0 + 8 * nb1 * (r + 1), off0 + 8 * nb1 * (r + 2),
                         key0 + starts[r], key0 + starts[r + 1], key0 + starts[r + 2], 0, 0, 0))
        jobs = np.array(rows, dtype=np.int64)
        check(lib().ksh_pair_algebra_batch(self.h, C.byref(g), C.cast(jobs.ctypes.data, C.POINTER(PairJob)), n))
        return BatchResult(g, off_rows, key_pool, starts, byte_caps, jobs[:, 12:15].tolist())

    def set_union_plan(self, a, b):
        """ksh_set_union_plan alone: a Pending with the operands, `out` (offsets filled, keys not yet allocated)
        and n_keys = |A | B|."""
        out = DeviceSet.empty_like_offsets(a.g, 0, self.device)
        total = C.c_int64()
        va, vb = a.view(), b.view()
        check(lib().ksh_set_union_plan(self.h, C.byref(a.g), C.byref(va), C.byref(vb),
                                       out.offsets.data_ptr(), C.byref(total)))
        out.n_keys = total.value
        return Pending(kind="union", a=a, b=b, out=out, n_keys=total.value)

    def set_union_write(self, plan, keys=None, g=None):
        """ksh_set_union_write on a Pending of set_union_plan; keys: a uint8 tensor of at least n_keys * key_bytes
        bytes (allocated when None); g replaces the planned geometry (the library refuses the mismatch)."""
        import torch

        g = plan.a.g if g is None else g
        if keys is None:
            keys = torch.empty(max(plan.n_keys * g.key_bytes, 16), dtype=torch.uint8, device=self.device)
        plan.out.keys = keys
        va, vb = plan.a.view(), plan.b.view()
        check(lib().ksh_set_union_write(self.h, C.byref(g), C.byref(va), C.byref(vb), keys.data_ptr()))
        return plan.out

    def set_union(self, a, b):
        """KmerSet::Add: A | B as a new DeviceSet."""
        return self.set_union_write(self.set_union_plan(a, b))

    def set_diff(self, a, b):
        out = C.c_int64()
        va, vb = a.view(), b.view()
        check(lib().ksh_set_diff(self.h, C.byref(a.g), C.byref(va), C.byref(vb), C.byref(out)))
        return out.value

    def pair_weights(self, sets, bucket_ids, pairs):
        g = sets[0].g
        views = (SetView * len(sets))(*[s.view() for s in sets])
        ids = np.ascontiguousarray(bucket_ids, dtype=np.int32)
        prs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1)
        n_pairs = prs.size // 2
        out = np.zeros(max(n_pairs, 1), dtype=np.int64)
        check(lib().ksh_pair_weights(
            self.h, C.byref(g), views, len(sets),
            ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size,
            prs.ctypes.data_as(C.POINTER(C.c_int32)), n_pairs,
            out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out[:n_pairs]


class DeviceKmerSetSet:
    """ksh_kss: KmerSetSet built on device (lib/core/kmer_set_set.h:109-427)."""

    def __init__(self, ctx, compacts, bucket_ids, canonical=True, max_iterations=-1, dist=None,
                 dist_device="cpu", g=None):
        """dist: an initialised torch.distributed module (one process per GPU) for the sharded
        build (ksh_kss_build_sharded): every rank passes the same inputs; the SPSS of a node
        lives on one rank (node_holder).  g: the geometry, needed only where there is no input to
        take it from (no inputs at all: a structure of 0 nodes)."""
        self.ctx, self.g, self.inputs = ctx, g if g is not None else compacts[0].g, list(compacts)
        self.canonical = bool(canonical)
        views = (SpssView * max(len(compacts), 1))(*[c.view() for c in compacts])
        ids = np.ascontiguousarray(bucket_ids, dtype=np.int32)
        h = C.c_void_p()
        if dist is None:
            check(lib().ksh_kss_build(ctx.h, C.byref(self.g), views, len(compacts),
                                      ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size, int(canonical),
                                      max_iterations, C.byref(h)))
        else:
            import torch

            world, rank = dist.get_world_size(), dist.get_rank()

            def gather(_user, send, count, recv):
                try:
                    mine = torch.from_numpy(np.ctypeslib.as_array(send, shape=(count,)).copy()).to(dist_device)
                    parts = [torch.empty_like(mine) for _ in range(world)]
                    dist.all_gather(parts, mine)
                    out = np.ctypeslib.as_array(recv, shape=(world * count,))
                    for r, part in enumerate(parts):
                        out[r * count:(r + 1) * count] = part.cpu().numpy()
                    return 0
                except Exception:  # a Python exception must not unwind through the C frames
                    import traceback

                    traceback.print_exc()
                    return 1

            self._gather = GATHER_FN(gather)  # keep the callback object alive
            check(lib().ksh_kss_build_sharded(ctx.h, C.byref(self.g), views, len(compacts),
                                              ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size,
                                              int(canonical), max_iterations, rank, world, self._gather, None,
                                              C.byref(h)))
        self.h = h

    def node_holder(self, i):
        """Rank holding node i's SPSS in a sharded build; -1: every rank does."""
        r = C.c_int32()
        check(lib().ksh_kss_node_holder(self.h, i, C.byref(r)))
        return r.value

    def close(self):
        if getattr(self, "h", None):
            lib().ksh_kss_destroy(self.h)
            self.h = None

    __del__ = close

    def size(self):
        n = C.c_int32()
        check(lib().ksh_kss_size(self.h, C.byref(n)))
        return n.value

    def node_strings(self, i):
        """SPSS strings of node i (downloaded)."""
        from . import synth

        sv = SpssView()
        check(lib().ksh_kss_node(self.h, i, C.byref(sv), None, None))
        n_words = (sv.n_bases + 31) // 32
        words = np.zeros(max(n_words, 1), dtype=np.uint64)
        lens = np.zeros(max(sv.n_strings, 1), dtype=np.uint32)
        if n_words:
            check(lib().ksh_ctx_memcpy_d2h(self.ctx.h, words.ctypes.data_as(C.c_void_p), sv.d_words, n_words * 8))
        if sv.n_strings:
            check(lib().ksh_ctx_memcpy_d2h(self.ctx.h, lens.ctypes.data_as(C.c_void_p), sv.d_lens, sv.n_strings * 4))
        return synth.unpack_strings(words[:n_words], lens[: sv.n_strings], self.g.k)

    def node_size(self, i):
        n = C.c_int64()
        check(lib().ksh_kss_node(self.h, i, None, None, C.byref(n)))
        return n.value

    def node_kmers(self, i):
        from . import synth

        v = SetView()
        check(lib().ksh_kss_node(self.h, i, None, C.byref(v), None))
        return self._download_set(v.d_offsets, v.d_keys, v.n_keys)

    def _download_set(self, d_off, d_keys, n_keys):
        from . import synth

        g = self.g
        nb = 1 << g.n_bucket_bits
        off = np.zeros(nb + 1, dtype=np.int64)
        kdt = KEY_DTYPE[g.key_bytes]
        keys = np.zeros(max(n_keys, 1), dtype=kdt)
        check(lib().ksh_ctx_memcpy_d2h(self.ctx.h, off.ctypes.data_as(C.c_void_p), d_off, (nb + 1) * 8))
        if n_keys:
            check(lib().ksh_ctx_memcpy_d2h(self.ctx.h, keys.ctypes.data_as(C.c_void_p), d_keys, n_keys * g.key_bytes))
        return synth.from_bucketed(off, keys[:n_keys], g.k, g.n_bucket_bits)

    def children(self, i):
        p, n = C.POINTER(C.c_int32)(), C.c_int32()
        check(lib().ksh_kss_children(self.h, i, C.byref(p), C.byref(n)))
        return [p[j] for j in range(n.value)]

    def meta(self):
        return lib().ksh_kss_meta(self.h).decode()

    def trace(self):
        ni, nc = C.c_int64(), C.c_int64()
        rows, crows, imp = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_float)()
        check(lib().ksh_kss_trace(self.h, C.byref(ni), C.byref(rows), C.byref(nc), C.byref(crows),
                                  C.byref(imp)))
        it = np.array([rows[i] for i in range(5 * ni.value)], dtype=np.int64).reshape(-1, 5)
        cp = np.array([crows[i] for i in range(4 * nc.value)], dtype=np.int64).reshape(-1, 4)
        im = np.array([imp[i] for i in range(nc.value)], dtype=np.float32)
        return it, cp, im

    def initial_weights(self):
        p, n = C.POINTER(C.c_int64)(), C.c_int64()
        check(lib().ksh_kss_initial_weights(self.h, C.byref(p), C.byref(n)))
        return np.array([p[i] for i in range(n.value)], dtype=np.int64)

    def stats(self):
        st = (C.c_int64 * 8)()
        check(lib().ksh_kss_stats(self.h, st))
        keys = ["initial_total_size", "final_total_size", "initial_spss_weight", "n_processed",
                "final_spss_weight", "packed_bytes", "length_bytes", "nodes"]
        out = dict(zip(keys, [int(x) for x in st]))
        ne, nk = C.c_int64(), C.c_int64()
        check(lib().ksh_kss_encode_counts(self.h, C.byref(ne), C.byref(nk)))
        out["n_encodes"], out["n_encoded_kmers"] = ne.value, nk.value
        check(lib().ksh_kss_weighed_counts(self.h, C.byref(ne), C.byref(nk)))
        out["n_weighed"], out["n_weighed_kmers"] = ne.value, nk.value
        ph = (C.c_double * 4)()
        check(lib().ksh_kss_phase_seconds(self.h, ph))
        out["phase_seconds"] = dict(zip(["decode_inputs", "weights", "merges", "encodes"], [float(x) for x in ph]))
        return out

    def get_size_and_hash(self, i):
        """(KmerSet::Size, KmerSet::Hash) of KmerSetSet::Get(i), computed on the device: what
        kmerset-multiple-compress --check compares per input set (src/kmerset-multiple-compress.cc:104-126)."""
        d_off, d_keys, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().ksh_kss_get(self.h, i, C.byref(d_off), C.byref(d_keys), C.byref(n)))
        try:
            v = SetView(d_off.value, d_keys.value, n.value)
            out = C.c_uint64()
            check(lib().ksh_set_hash(self.ctx.h, C.byref(self.g), C.byref(v), C.byref(out)))
            return n.value, out.value
        finally:
            dev = self.ctx.device.index
            lib().ksh_free(dev, d_off)
            lib().ksh_free(dev, d_keys)

    def get_kmers(self, i):
        """KmerSetSet::Get(i) as a sorted uint64 array (downloaded)."""
        d_off, d_keys, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().ksh_kss_get(self.h, i, C.byref(d_off), C.byref(d_keys), C.byref(n)))
        try:
            return self._download_set(d_off, d_keys, n.value)
        finally:
            dev = self.ctx.device.index
            lib().ksh_free(dev, d_off)
            lib().ksh_free(dev, d_keys)


QROUTE_SEARCH, QROUTE_JOIN, QROUTE_OVERSIZE, QROUTE_CHUNKED, QROUTE_SEQ_PASSES = 1, 2, 4, 8, 16
QROUTE_PAIR_SPLIT, QROUTE_PAIR_FLUSH, QROUTE_CLASS_SPILL = 32, 64, 128
CLASS_NONE = 0xFFFFFFFF  # KSH_CLASS_NONE: the id of a k-mer whose row the class table does not hold


class KssIndex:
    """ksh_kss_index: which nodes' Get(i) hold each query k-mer (kmer_set_set.h:433-454), for every node i."""

    def __init__(self, ctx, h, keep, borrowed=None, g=None, canonical=True):
        self.ctx, self.h, self._keep, self._borrowed, self.g = ctx, h, keep, borrowed, g
        self.canonical = bool(canonical)  # (what the node sets were decoded with: colored_unitigs encodes with it)
        n, w, b = C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().ksh_kss_index_info(h, C.byref(n), C.byref(w), C.byref(b)))
        self.n_nodes, self.words = n.value, w.value

    @classmethod
    def from_kss(cls, dkss):
        """Borrows the resident node sets of a built DeviceKmerSetSet (kept alive by the index)."""
        h = C.c_void_p()
        check(lib().ksh_kss_index_from_kss(dkss.h, C.byref(h)))
        return cls(dkss.ctx, h, dkss, borrowed=dkss, g=dkss.g, canonical=getattr(dkss, "canonical", True))

    def _handle(self):
        """The live index; an index whose borrowed structure was closed is closed too (its node sets are gone)."""
        if self._borrowed is not None and getattr(self._borrowed, "h", None) is None:
            self.close()
            raise KshError(KSH_FAILED_PRECONDITION, "the KmerSetSet this index borrows its node sets from is closed")
        if not getattr(self, "h", None):
            raise KshError(KSH_FAILED_PRECONDITION, "the index is closed")
        return self.h

    @classmethod
    def from_nodes(cls, ctx, compacts, children, canonical=True):
        """From node containers (DeviceSpss) and children lists (children[i] = node i's children, or a dict
        {i: [...]} as KmerSetSet::Load has): the index decodes every node."""
        n = len(compacts)
        if isinstance(children, dict):
            children = [children.get(i, []) for i in range(n)]
        offs = np.zeros(n + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(children[i]) for i in range(n)]) if n else []
        ids = np.ascontiguousarray([c for i in range(n) for c in children[i]] or [0], dtype=np.int32)
        views = (SpssView * max(n, 1))(*[c.view() for c in compacts])
        h = C.c_void_p()
        check(lib().ksh_kss_index_create(ctx.h, C.byref(compacts[0].g if n else Geom()), views, n,
                                          offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                          ids.ctypes.data_as(C.POINTER(C.c_int32)), int(canonical), C.byref(h)))
        return cls(ctx, h, list(compacts), g=compacts[0].g if n else None, canonical=canonical)

    def query(self, kmers, canonicalize=True, route=0, packed=False):
        """Rows for the 2K-bit patterns `kmers` (numpy, or a device torch tensor of int64/uint64): an n x n_nodes
        bool array, or with packed=True the n x W uint64 rows (a device tensor stays on the device)."""
        import torch

        with torch.cuda.stream(self.ctx.stream):   # (another context made since may have become torch's current stream)
            return self._query(kmers, canonicalize, route, packed)

    def _query(self, kmers, canonicalize, route, packed):
        import torch

        on_device = isinstance(kmers, torch.Tensor)
        if on_device:
            q = kmers.contiguous()
            if q.dtype != torch.int64:
                q = q.view(torch.int64) if q.element_size() == 8 else q.to(torch.int64)
            q = q.to(self.ctx.device)
        else:
            q = torch.from_numpy(np.ascontiguousarray(kmers, dtype=np.uint64).view(np.int64).copy()).to(self.ctx.device)
        n = q.numel()
        rows = torch.empty((max(n, 1), self.words), dtype=torch.int64, device=self.ctx.device)
        check(lib().ksh_kss_index_query(self._handle(), q.data_ptr() if n else None, n, int(bool(canonicalize)), int(route),
                                        rows.data_ptr()))
        rows = rows[:n]
        if packed:
            return rows if on_device else rows.cpu().numpy().view(np.uint64)
        host = rows.cpu().numpy().view(np.uint64)
        bits = np.unpackbits(host.view(np.uint8).reshape(n, self.words * 8), axis=1, bitorder="little")
        return bits[:, : self.n_nodes].astype(bool)

    def seq_hits(self, seqs, canonicalize=True, route=0, pass_positions=0, device=False):
        """ksh_seq_hits: for every sequence of `seqs` (a DeviceSpss, or a list of str over ACGT, each at least K
        long, uploaded through DeviceSpss.from_strings) and every node i, the number of the sequence's k-mer
        positions whose k-mer is in Get(i): a uint32 array [n_seqs, n_nodes] (numpy; device=True: a torch.uint32
        tensor that stays on the device)."""
        import torch

        with torch.cuda.stream(self.ctx.stream):
            return self._seq_hits(seqs, canonicalize, route, pass_positions, device)

    def _seq_hits(self, seqs, canonicalize, route, pass_positions, device):
        import torch

        h = self._handle()
        if not isinstance(seqs, DeviceSpss):
            seqs = DeviceSpss.from_strings(self.g, list(seqs), self.ctx.device)
        n = seqs.n_strings
        hits = torch.empty((max(n, 1), self.n_nodes), dtype=torch.int32, device=self.ctx.device)
        view = seqs.view()
        check(lib().ksh_seq_hits(C.byref(view), h, int(bool(canonicalize)), int(route), int(pass_positions),
                                 hits.data_ptr()))
        hits = hits[:n]
        return hits.view(torch.uint32) if device else hits.cpu().numpy().view(np.uint32)

    def pair_counts(self, cols=None, flush_rows=0, device=False, with_distinct=False):
        """ksh_kss_pair_counts: counts[a, b] = |Get(cols[a]) & Get(cols[b])|, exact, as an int64 array
        [n_cols, n_cols] (numpy; device=True: a torch tensor that stays on the device).  cols: up to 128 distinct
        node ids in any order; None: all nodes in order (an index of more than 128 nodes is refused: name the
        columns, two blocks of at most 64 per call).  with_distinct=True returns (counts, the number of distinct
        k-mers held by any node of the index)."""
        import torch

        with torch.cuda.stream(self.ctx.stream):
            return self._pair_counts(cols, flush_rows, device, with_distinct)

    def _pair_counts(self, cols, flush_rows, device, with_distinct):
        import torch

        h = self._handle()
        if cols is None:
            n, ids = self.n_nodes, None
        else:
            arr = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
            n = int(arr.size)
            ids = (arr if n else np.zeros(1, dtype=np.int32)).ctypes.data_as(C.POINTER(C.c_int32))  # (never NULL)
        side = min(max(n, 1), 128)  # (what the call refuses is never written)
        counts = torch.empty((side, side), dtype=torch.int64, device=self.ctx.device)
        distinct = C.c_int64()
        check(lib().ksh_kss_pair_counts(ids, n, h, int(flush_rows), counts.data_ptr(),
                                        C.byref(distinct) if with_distinct else None))
        out = counts if device else counts.cpu().numpy()
        return (out, distinct.value) if with_distinct else out

    def _selection(self, cols, min_count, max_count, require, exclude):
        """(ksh_kss_selection, n_cols, the arrays it points to -- keep them alive for the call)."""
        def ids(x):
            arr = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)
            return arr, int(arr.size), (arr if arr.size else np.zeros(1, dtype=np.int32)).ctypes.data_as(
                C.POINTER(C.c_int32))  # (never NULL: an empty list is a count of 0)
        if cols is None:
            keep_c, n_cols, p_cols = None, self.n_nodes, None
        else:
            keep_c, n_cols, p_cols = ids(cols)
        keep_r, n_req, p_req = ids(require)
        keep_x, n_exc, p_exc = ids(exclude)
        sel = Selection(C.sizeof(Selection), p_cols, n_cols if cols is not None else 0, int(min_count),
                        0 if max_count is None else int(max_count), p_req, n_req, p_exc, n_exc)
        return sel, n_cols, (keep_c, keep_r, keep_x)

    def select_count(self, cols=None, min_count=1, max_count=None, require=(), exclude=(), offsets=True,
                     size=True, spectrum=False):
        """ksh_kss_select_count, the raw call: (offsets, n_keys, spectrum) of the selection -- a device int64
        tensor [2^N + 1], an int, an np.int64 array [n_cols + 1] -- each None where its flag is False."""
        import torch

        with torch.cuda.stream(self.ctx.stream):
            h = self._handle()
            sel, n_cols, keep = self._selection(cols, min_count, max_count, require, exclude)
            off = torch.empty((1 << self.g.n_bucket_bits) + 1, dtype=torch.int64, device=self.ctx.device) \
                if offsets else None
            n = C.c_int64()
            spec = np.zeros(min(max(n_cols, 1), 128) + 1, dtype=np.int64)  # (what the call refuses is never written)
            check(lib().ksh_kss_select_count(C.byref(sel), h, off.data_ptr() if offsets else None,
                                             C.byref(n) if size else None,
                                             spec.ctypes.data_as(C.POINTER(C.c_int64)) if spectrum else None))
            del keep
            return off, (n.value if size else None), (spec if spectrum else None)

    def select_write(self, offsets, n_keys, keys, cols=None, min_count=1, max_count=None, require=(), exclude=()):
        """ksh_kss_select_keys, the raw call: writes the selection's keys into `keys` (a device tensor of at least
        n_keys keys, or None with n_keys == 0) at the bucket offsets `offsets`; n_keys is the capacity in keys."""
        import torch

        with torch.cuda.stream(self.ctx.stream):
            h = self._handle()
            sel, n_cols, keep = self._selection(cols, min_count, max_count, require, exclude)
            check(lib().ksh_kss_select_keys(C.byref(sel), h, offsets.data_ptr() if offsets is not None else None,
                                            int(n_keys), keys.data_ptr() if keys is not None else None))
            del keep

    def select(self, cols=None, min_count=1, max_count=None, require=(), exclude=()):
        """The k-mers q held by any node with min_count <= c(q) <= max_count (c(q) = the number of a with q in
        Get(cols[a]); max_count None: n_cols), in Get(r) for every r of require and in no Get(x) of exclude, as a
        DeviceSet that every other call accepts.  cols: up to 128 distinct node ids (None: all nodes); require and
        exclude: ids out of cols.  The core of cols is min_count = len(cols); the k-mers private to s are
        require=[s], max_count=1."""
        import torch

        off, n, _ = self.select_count(cols, min_count, max_count, require, exclude)
        with torch.cuda.stream(self.ctx.stream):
            keys = torch.empty(max(n * self.g.key_bytes, 16), dtype=torch.uint8, device=self.ctx.device)
        self.select_write(off, n, keys, cols, min_count, max_count, require, exclude)
        return DeviceSet(self.g, off, keys, n)

    def spectrum(self, cols=None):
        """np.int64[n_cols + 1]: element m is the number of distinct k-mers of the whole structure that exactly m of
        the sets Get(cols[a]) hold (element 0: those that only nodes outside cols hold)."""
        return self.select_count(cols, offsets=False, size=False, spectrum=True)[2]

    def color_classes(self, cols=None, capacity=None):
        """ksh_kss_color_classes: (rows, counts) -- rows np.uint64[n, 2], one distinct membership pattern over the
        columns per line (bit a % 64 of rows[c, a // 64]: the class's k-mers are in Get(cols[a])), counts np.int64[n]
        the distinct k-mers of the structure with exactly that pattern, ascending by (rows[c, 1], rows[c, 0]).  Row
        zero counts the k-mers that only nodes outside cols hold.  cols: up to 128 distinct node ids (None: all
        nodes).  capacity None: room for min(2^n_cols, 2^16) classes, times 4 for as long as the call answers that
        there are more, up to min(2^n_cols, 2^24), where the refusal is raised; a given capacity is tried once."""
        import torch

        with torch.cuda.stream(self.ctx.stream):   # (results are read on the context's stream, not torch's current)
            h = self._handle()
            if cols is None:
                n, ids, keep = self.n_nodes, None, None
            else:
                keep = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
                n = int(keep.size)
                ids = (keep if n else np.zeros(1, dtype=np.int32)).ctypes.data_as(C.POINTER(C.c_int32))  # (never NULL)
            top = 1 << min(max(n, 0), 24)  # min(2^n_cols, 2^24)
            cap = min(top, 1 << 16) if capacity is None else int(capacity)
            while True:
                room = min(max(cap, 1), 1 << 24)  # (what the call refuses is never written)
                rows = np.zeros((room, 2), dtype=np.uint64)
                counts = np.zeros(room, dtype=np.int64)
                got = C.c_int64()
                rc = lib().ksh_kss_color_classes(ids, n if cols is not None else 0, h, cap,
                                                 rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(got))
                if rc == KSH_FAILED_PRECONDITION and got.value == cap + 1 and capacity is None and cap < top:
                    cap = min(4 * cap, top)
                    continue
                check(rc)
                del keep
                return rows[:got.value].copy(), counts[:got.value].copy()

    def select_class_ids(self, offsets, n_keys, rows, keys=None, ids=None, cols=None, min_count=1, max_count=None,
                         require=(), exclude=(), allow_unmatched=False):
        """ksh_kss_select_class_ids, the raw call: writes the selection's keys into `keys` (a device tensor of at
        least n_keys keys, or None: only the ids are written) and beside each key the position of its row in the
        class table `rows` (np.uint64[n, 2] as color_classes returns it, or an ascending subset) into `ids` (a
        device int32 tensor of at least n_keys values, or None with n_keys == 0).  A k-mer whose row is not in the
        table is refused, or with allow_unmatched gets CLASS_NONE (-1 as int32); the number of such k-mers is
        returned with allow_unmatched, otherwise None."""
        import torch

        with torch.cuda.stream(self.ctx.stream):
            h = self._handle()
            sel, n_cols, keep = self._selection(cols, min_count, max_count, require, exclude)
            table = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
            missing = C.c_int64()
            check(lib().ksh_kss_select_class_ids(
                C.byref(sel), h, table.ctypes.data_as(C.POINTER(C.c_uint64)) if table is not None else None,
                table.size // 2 if table is not None else 0, offsets.data_ptr() if offsets is not None else None,
                int(n_keys), keys.data_ptr() if keys is not None else None,
                ids.data_ptr() if ids is not None else None, C.byref(missing) if allow_unmatched else None))
            del keep
            return missing.value if allow_unmatched else None

    def select_classes(self, cols=None, min_count=1, max_count=None, require=(), exclude=(), rows=None,
                       allow_unmatched=False):
        """The selection of select() with the colour class of every k-mer: (DeviceSet, ids, rows, counts).  ids is a
        device int32 tensor aligned with the set's keys: ids[p] is the position in `rows` of the membership pattern
        of key p over cols, or -1 (CLASS_NONE) where allow_unmatched lets a pattern be absent from the table.
        rows None: the table is color_classes(cols), returned with its counts; a given table (np.uint64[n, 2],
        ascending as color_classes returns it, or a subset of it) is returned as it is, with counts None.  The union
        selection with the whole table is a coloured de Bruijn graph: its k-mers, a class per k-mer, the classes."""
        import torch

        counts = None
        if rows is None:
            rows, counts = self.color_classes(cols)
        off, n, _ = self.select_count(cols, min_count, max_count, require, exclude)
        with torch.cuda.stream(self.ctx.stream):
            keys = torch.empty(max(n * self.g.key_bytes, 16), dtype=torch.uint8, device=self.ctx.device)
            ids = torch.empty(max(n, 1), dtype=torch.int32, device=self.ctx.device)
        if n == 0 and len(rows) == 0:  # (an index without k-mers: no class to name, and the call takes no empty table)
            return DeviceSet(self.g, off, keys, 0), ids[:0], rows, counts
        self.select_class_ids(off, n, rows, keys, ids, cols, min_count, max_count, require, exclude,
                              allow_unmatched=allow_unmatched)
        return DeviceSet(self.g, off, keys, n), ids[:n], rows, counts

    def class_runs_raw(self, seqs, rows, capacity, offsets=None, start=None, cls=None, cols=None, canonicalize=True,
                       route=0, pass_positions=0, allow_unmatched=True):
        """ksh_seq_class_runs, one call: (rc, n_runs, n_unmatched or None).  seqs: a DeviceSpss; offsets, start, cls:
        device tensors or None.  rc is KSH_OK or KSH_FAILED_PRECONDITION (too small a capacity, or a row the table
        does not hold without allow_unmatched: the message is ksh_last_error); anything else is raised."""
        import torch

        with torch.cuda.stream(self.ctx.stream):
            h = self._handle()
            keep = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
            ids = None if cols is None else (keep if keep.size else np.zeros(1, dtype=np.int32)).ctypes.data_as(
                C.POINTER(C.c_int32))  # (never NULL)
            table = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
            req = SeqPaint(C.sizeof(SeqPaint), ids, 0 if cols is None else int(keep.size), int(bool(canonicalize)),
                           None if table is None else table.ctypes.data_as(C.POINTER(C.c_uint64)),
                           0 if table is None else table.size // 2, int(route), int(pass_positions))
            view = seqs.view()
            n_runs, missing = C.c_int64(-1), C.c_int64()
            rc = lib().ksh_seq_class_runs(C.byref(view), h, C.byref(req), int(capacity),
                                          offsets.data_ptr() if offsets is not None else None,
                                          start.data_ptr() if start is not None else None,
                                          cls.data_ptr() if cls is not None else None, C.byref(n_runs),
                                          C.byref(missing) if allow_unmatched else None)
            del keep, table
            if rc not in (KSH_OK, KSH_FAILED_PRECONDITION):
                check(rc)
            return rc, n_runs.value, (missing.value if allow_unmatched else None)

    def class_runs(self, seqs, rows, cols=None, canonicalize=True, route=0, pass_positions=0, capacity=None,
                   allow_unmatched=True):
        """ksh_seq_class_runs: the sequences of `seqs` (a DeviceSpss, or a list of str over ACGT, each at least K long)
        cut into runs of consecutive k-mer positions of one colour class.  rows: a class table np.uint64[n, 2] as
        color_classes(cols) returns it, or an ascending subset of it.  Returns (run_offsets, run_start, run_class,
        n_unmatched): device tensors int64[n_seqs + 1], int32[n_runs], int32[n_runs] -- the runs of sequence s are
        run_offsets[s] .. run_offsets[s + 1), run r begins at position run_start[r] of its sequence and has class
        run_class[r], -1 (CLASS_NONE) where the table does not hold the position's row -- and the number of such
        positions (None, and a refusal if there are any, with allow_unmatched=False).  capacity None: one call counts
        the runs and a second one writes them; a given capacity is tried once."""
        import torch

        if not isinstance(seqs, DeviceSpss):
            seqs = DeviceSpss.from_strings(self.g, list(seqs), self.ctx.device)
        kw = dict(cols=cols, canonicalize=canonicalize, route=route, pass_positions=pass_positions,
                  allow_unmatched=allow_unmatched)
        with torch.cuda.stream(self.ctx.stream):
            off = torch.zeros(seqs.n_strings + 1, dtype=torch.int64, device=self.ctx.device)
        if capacity is None:
            rc, capacity, _ = self.class_runs_raw(seqs, rows, 0, off, **kw)
            check(rc)
        capacity = int(capacity)
        with torch.cuda.stream(self.ctx.stream):
            start = torch.empty(max(capacity, 1), dtype=torch.int32, device=self.ctx.device)
            cls = torch.empty(max(capacity, 1), dtype=torch.int32, device=self.ctx.device)
        rc, n_runs, missing = self.class_runs_raw(seqs, rows, capacity, off, start if capacity else None,
                                                  cls if capacity else None, **kw)
        check(rc)
        n_runs = min(n_runs, capacity)  # (capacity 0 only counts: the offsets are whole, the runs are not asked for)
        return off, start[:n_runs], cls[:n_runs], missing

    def paint(self, seqs, cols=None, canonicalize=True, route=0, pass_positions=0, allow_unmatched=True):
        """class_runs with the whole table of the columns: (run_offsets, run_start, run_class, n_unmatched, rows,
        counts), rows and counts being color_classes(cols).  A k-mer that no node of the index holds has the zero
        row, which the table only holds if some k-mer of the structure lies outside every column: such positions are
        -1 in run_class and counted in n_unmatched."""
        rows, counts = self.color_classes(cols)
        out = self.class_runs(seqs, rows, cols, canonicalize, route, pass_positions, None, allow_unmatched)
        return out + (rows, counts)

    def colored_unitigs(self, cols=None, mode=0, route=0, pass_positions=0):
        """The coloured de Bruijn graph of the columns as monochromatic strings: (spss, string_class, rows, counts).
        spss is a DeviceSpss whose strings hold every k-mer that a column holds exactly once, all k-mers of a string
        in one colour class; string_class is a device int32 tensor [n_strings], string r has class string_class[r] of
        the table rows, counts = color_classes(cols).  The union selection with its classes (select_classes) is
        encoded (Context.spss_encode with `mode` and the index's canonical flag), the strings are painted
        (class_runs with `route` and `pass_positions`) and cut at the runs (Context.spss_cut); nothing but the counts
        those calls return leaves the device."""
        ds, _, rows, counts = self.select_classes(cols)
        if ds.n_keys == 0:
            import torch

            with torch.cuda.stream(self.ctx.stream):
                none = torch.zeros(0, dtype=torch.int32, device=self.ctx.device)
            return DeviceSpss.from_strings(self.g, [], self.ctx.device), none, rows, counts
        uncut = self.ctx.spss_encode(ds, mode=mode, canonical=self.canonical)
        off, start, cls, _ = self.class_runs(uncut, rows, cols, canonicalize=self.canonical, route=route,
                                             pass_positions=pass_positions, allow_unmatched=False)
        return self.ctx.spss_cut(uncut, off, start), cls, rows, counts

    def colored_graph(self, cols=None, route=0, pass_positions=0):
        """The coloured compacted de Bruijn graph of the columns, nodes and edges: (spss, string_class, rows, counts,
        link_offsets, link_to).  The first four are colored_unitigs(cols, mode=1, route, pass_positions): mode 1 makes
        the strings pieces of unitigs, so the links between their ends are all the edges of the graph.  The last two
        are Context.spss_links of those strings with the index's canonical flag."""
        spss, cls, rows, counts = self.colored_unitigs(cols, mode=1, route=route, pass_positions=pass_positions)
        off, link_to = self.ctx.spss_links(spss, canonical=self.canonical)
        return spss, cls, rows, counts, off, link_to

    def colored_bubbles(self, cols=None, max_arm=8, route=0, pass_positions=0):
        """The bubbles of the coloured graph of the columns: the six values of colored_graph(cols, route,
        pass_positions) followed by the four of Context.link_bubbles on its links with the graph's classes and rows:
        (spss, string_class, rows, counts, link_offsets, link_to, ends, arm_offsets, arm_strings, arm_rows).  Bit a
        of an arm's row is column cols[a].  The links are taken as canonical ones: an index built without the
        canonical flag is refused as soon as its graph has a link."""
        spss, cls, rows, counts, off, link_to = self.colored_graph(cols, route=route, pass_positions=pass_positions)
        if spss.n_strings == 0:  # (no string, no class to name: the call takes no empty table)
            import torch

            bubbles = self.ctx.link_bubbles(off, link_to, max_arm)[:3]
            with torch.cuda.stream(self.ctx.stream):
                bubbles += (torch.empty((0, 2), dtype=torch.uint64, device=self.ctx.device),)
        else:
            bubbles = self.ctx.link_bubbles(off, link_to, max_arm, string_class=cls, rows=rows)
        return (spss, cls, rows, counts, off, link_to) + bubbles

    def colored_variants(self, reference, cols=None, max_arm=8, route=0, pass_positions=0):
        """The bubbles of the coloured graph with the graph placed on a reference: the ten values of
        colored_bubbles(cols, max_arm, route, pass_positions) followed by (where, count) = Context.seq_locate of the
        graph's strings in `reference` with the index's canonical flag.  reference: a DeviceSpss (for instance from
        Context.fasta_fragments) or a list of strings over ACGT of at least K bases each.  capi.place_bubbles and
        capi.write_vcf make records and VCF text of the twelve values."""
        out = self.colored_bubbles(cols, max_arm=max_arm, route=route, pass_positions=pass_positions)
        if not isinstance(reference, DeviceSpss):
            reference = DeviceSpss.from_strings(self.g, list(reference), self.ctx.device)
        return out + self.ctx.seq_locate(out[0], reference, canonical=self.canonical)

    @staticmethod
    def class_matrix(rows, n_cols):
        """bool[n, n_cols] of the rows color_classes returned: element [c, a] is bit a of class c."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
        bits = np.unpackbits(rows.view(np.uint8).reshape(rows.shape[0], 16), axis=1, bitorder="little")
        return bits[:, :int(n_cols)].astype(bool)

    def jaccard(self, cols=None):
        """Exact Jaccard similarities c_ab / (c_aa + c_bb - c_ab) of the sets Get(cols[a]), a float64 numpy array
        computed on the host from pair_counts(cols).  Two empty sets (0 / 0) are defined as 1.0."""
        c = self.pair_counts(cols).astype(np.float64)
        d = np.diag(c)
        union = d[:, None] + d[None, :] - c
        return np.where(union > 0, c / np.where(union > 0, union, 1.0), 1.0)

    def routes(self):
        bits = C.c_uint32()
        check(lib().ksh_kss_index_routes(self._handle(), C.byref(bits)))
        return bits.value

    def info(self):
        n, w, b = C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().ksh_kss_index_info(self._handle(), C.byref(n), C.byref(w), C.byref(b)))
        return {"n_nodes": n.value, "words_per_row": w.value, "resident_bytes": b.value}

    def close(self):
        # (once its context is closed, the index's buffers went with the context's pool)
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().ksh_kss_index_destroy(self.h)
        self.h = None
        self._keep = self._borrowed = None

    __del__ = close


class Comm:
    """ksh_comm: the transport of the owner-sharded build.  backend "nccl": RCCL inside the library on
    device buffers (rank 0 draws the id, torch.distributed carries its 128 bytes to the others);
    anything else: the caller-supplied functions, here gloo through host memory (rehearsals with
    several ranks on one GPU, where RCCL cannot run)."""

    def __init__(self, ctx, dist, coll_dev):
        import torch

        self.ctx, self.dist = ctx, dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        h = C.c_void_p()
        if dist.get_backend() == "nccl":
            buf = C.create_string_buffer(KSH_COMM_ID_BYTES)
            if self.rank == 0:
                check(lib().ksh_comm_unique_id(buf))
            t = torch.tensor(list(buf.raw), dtype=torch.uint8, device=coll_dev)
            dist.broadcast(t, 0)
            raw = bytes(t.cpu().tolist())
            check(lib().ksh_comm_create_rccl(ctx.h, self.rank, self.world, raw, C.byref(h)))
            self.kind = "rccl"
        else:
            dev = ctx.device.index

            def d2h(ptr, n):
                a = np.empty(n, dtype=np.uint8)
                if n:
                    check(lib().ksh_ctx_memcpy_d2h(ctx.h, a.ctypes.data_as(C.c_void_p), ptr, n))
                return torch.from_numpy(a)

            def h2d(ptr, t):
                a = t.numpy()
                if a.size:
                    check(lib().ksh_ctx_memcpy_h2d(ctx.h, ptr, a.ctypes.data_as(C.c_void_p), a.size))

            def guarded(f):
                def g(*args):
                    try:
                        f(*args)
                        return 0
                    except Exception:  # a Python exception must not unwind through the C frames
                        import traceback

                        traceback.print_exc()
                        return 1
                return g

            @guarded
            def allgather(_u, d_send, d_recv, n):
                mine = d2h(d_send, n)
                parts = [torch.empty_like(mine) for _ in range(self.world)]
                dist.all_gather(parts, mine)
                h2d(d_recv, torch.cat(parts))

            @guarded
            def send(_u, d_buf, n, peer):
                dist.send(d2h(d_buf, n), peer)

            @guarded
            def recv(_u, d_buf, n, peer):
                t = torch.empty(n, dtype=torch.uint8)
                dist.recv(t, peer)
                h2d(d_buf, t)

            def abort(_u):
                # a rank gives the build up where it cannot follow the protocol: the transport's own abort, if any
                f = getattr(dist, "abort", None)
                if f is not None:
                    f()

            self._keep = (COMM_ALLGATHER_FN(allgather), COMM_P2P_FN(send), COMM_P2P_FN(recv), COMM_ABORT_FN(abort))
            self._fns = CommFns(C.sizeof(CommFns), None, *self._keep)
            check(lib().ksh_comm_create_custom(ctx.h, self.rank, self.world, C.byref(self._fns), C.byref(h)))
            self.kind = "custom"
        self.h = h

    def ranks_seen(self):
        """Collective: the ranks whose ids arrived here through the transport's all-gather."""
        n = C.c_int32()
        check(lib().ksh_comm_ranks_seen(self.h, C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "h", None):
            lib().ksh_comm_destroy(self.h)
            self.h = None

    __del__ = close


def block_owners(n_sets, world):
    """Input i lives on rank i * world // n_sets: contiguous blocks (neighbours in the input order are
    the likeliest to merge first)."""
    return [i * world // n_sets for i in range(n_sets)]


class OwnedKmerSetSet(DeviceKmerSetSet):
    """ksh_kss_build_owned: the multi-GPU KmerSetSet in which a node's set and SPSS live on one rank.
    compacts[i] is the input's DeviceSpss on its owner and None elsewhere."""

    def __init__(self, ctx, compacts, bucket_ids, dist, coll_dev, canonical=True, max_iterations=-1, owners=None,
                 comm=None, g=None):
        """g: the geometry, for a rank that owns no input to take it from (fewer inputs than ranks)."""
        self.ctx, self.dist, self.coll_dev = ctx, dist, coll_dev
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.owners = list(owners) if owners is not None else block_owners(len(compacts), self.world)
        mine = [c for c in compacts if c is not None]
        if not mine and g is None:
            raise ValueError("rank %d owns no input: pass the geometry (g=)" % self.rank)
        self.g, self.inputs = g if g is not None else mine[0].g, list(compacts)
        self.canonical = bool(canonical)
        for i, c in enumerate(compacts):
            if (c is not None) != (self.owners[i] == self.rank):
                raise ValueError("input %d: the container must be given on its owner (rank %d) only" % (i, self.owners[i]))
        views = (SpssView * max(len(compacts), 1))(*[c.view() if c is not None else SpssView(None, None, 0, 0)
                                                     for c in compacts])
        own = np.ascontiguousarray(self.owners, dtype=np.int32)
        ids = np.ascontiguousarray(bucket_ids, dtype=np.int32)
        self._own_comm = comm is None
        self.comm = comm if comm is not None else Comm(ctx, dist, coll_dev)
        h = C.c_void_p()
        check(lib().ksh_kss_build_owned(ctx.h, self.comm.h, C.byref(self.g), views, len(compacts),
                                        own.ctypes.data_as(C.POINTER(C.c_int32)),
                                        ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size, int(canonical),
                                        max_iterations, C.byref(h)))
        self.h = h
        self._table = None

    def close(self):
        DeviceKmerSetSet.close(self)
        if getattr(self, "_own_comm", False) and getattr(self, "comm", None) is not None:
            self.comm.close()
            self.comm = None

    __del__ = close

    def comm_stats(self):
        st = (C.c_int64 * 8)()
        check(lib().ksh_kss_comm_stats(self.h, st))
        return dict(zip(["p2p_bytes_sent", "p2p_bytes_received", "p2p_sets", "gather_bytes", "checks_deferred",
                         "rollbacks", "sets_migrated", "weight_gathers"], [int(x) for x in st]))

    def node_table(self):
        """(size, XOR hash) of every node, from the ranks that hold them (one all-gather)."""
        import torch

        if self._table is None:
            n = self.size()
            mine = np.zeros((n, 2), dtype=np.int64)
            for i in range(n):
                if self.node_holder(i) != self.rank:
                    continue
                v = SetView()
                check(lib().ksh_kss_node(self.h, i, None, C.byref(v), None))
                hsh = C.c_uint64()
                check(lib().ksh_set_hash(self.ctx.h, C.byref(self.g), C.byref(v), C.byref(hsh)))
                mine[i] = (v.n_keys, np.uint64(hsh.value).astype(np.int64))
            t = torch.from_numpy(mine).to(self.coll_dev)
            self.dist.all_reduce(t)          # every node is reported by exactly one rank
            self._table = t.cpu().numpy()
        return self._table

    def get_size_and_hash(self, i):
        """(Size, Hash) of Get(i): the nodes reachable from i are pairwise disjoint (every merge splits a
        set into its remainder and the new child), so the size is their sum and the hash their XOR."""
        tab = self.node_table()
        seen, todo = set(), [i]
        while todo:
            cur = todo.pop()
            if cur in seen:
                continue
            seen.add(cur)
            todo.extend(self.children(cur))
        size, hsh = 0, 0
        for node in seen:
            size += int(tab[node, 0])
            hsh ^= int(np.int64(tab[node, 1]).astype(np.uint64))
        return size, hsh
