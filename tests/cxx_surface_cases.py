"""Shared table of tests/test_cxx_surface_host.py (CPU) and tests/test_gpu_cxx_surface.py (GPU): the small matrices, the alpha / beta pairs and the
call order of tests/cxx/surface_driver.cpp, which runs every entry of the C++ surface (include/api/spmv.h, include/spmv_acc_strategies.hpp) on them.

The matrices sit at the edges of the two-width split (k_vector_row.hip: vector_tile_kernel and vector_row_kernel<1|4> with row_split = m / 2 and one lane
width per half), which adaptive_vec_row_sparse_spmv launches by hand and `adaptive` reaches under tunables adaptive_timed = 0, adaptive_split = 1:
m = 1 (the first half has no rows), odd m, an empty half, the width pair 2 / 64, rows longer than one 2048-product tile on both sides of m / 2, m around
the 256 rows a width-2 workgroup holds, rectangular shapes, no entries at all.  Row lengths are fixed, columns uniform in [0, n), values standard
normal, every case from its own fixed seed.

PLAIN MODULE, not a conftest: imported by name."""
import struct
import zlib

import numpy as np

from spmv_acc_amd import synth

INT_MAX = 2 ** 31 - 1

# (alpha, beta).  Where beta == 0 the y handed to the entry is all NaN: beta == 0 never reads y (tests/special_values.py), so a NaN that comes back
# is a failure.
ALPHA_BETA = [(1.0, 1.0), (-0.75, 0.0), (2.0, 0.5), (0.0, 1.5)]


def _from_lengths(tag, lens, n):
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    lens = np.asarray(lens, dtype=np.int64)
    rowptr = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    nnz = int(rowptr[-1])
    cols = rng.integers(0, n, size=nnz).astype(np.int32)
    return rowptr.astype(np.int32), cols, rng.standard_normal(nnz)


def _straddle_lengths():
    lens = np.zeros(1500, dtype=np.int64)
    lens[749], lens[750], lens[1400:] = 20000, 4097, 5
    return lens


def _build():
    cases = [
        ("one", [1], 1),                                        # half = 0: the first half has no blocks
        ("one_long", [5001], 64),                               # a row of three tiles with half = 0
        ("two_empty_first", [0, 300], 64),                      # empty first half: avg0 = 0 gives the row cap; w1 = 64
        ("three", [7, 0, 1], 4),                                # odd m, half = 1, nnz not a multiple of 4
        ("odd_widths", [1] * 50 + [40] * 51, 101),              # odd m; widths 2 against 8 (tile) / 32 (classic)
        ("heavy_first", [600] * 50 + [0] * 50, 100),            # the second half empty: width 64 against 2
        ("no_entries", [0] * 100, 5),                           # scale-only; colindex / value are empty
        ("straddle", _straddle_lengths(), 2000),                # multi-tile rows on both sides of m / 2 = 750; halves 20000 against 4597
        ("tile_edges", [1024] * 40, 500),                       # rows ending on tile boundaries
        ("rpb_512", [5] * 512, 512), ("rpb_513", [5] * 513, 513), ("rpb_514", [5] * 514, 514),  # half = 256, 256, 257: the width-2 workgroup's rows
    ]
    out = [(tag,) + _from_lengths(tag, lens, n) + (n,) for tag, lens, n in cases]
    out.append(("wide",) + synth.random_csr(300, 900, 100, seed=701, kind="uniform") + (900,))      # rectangular, n > m
    out.append(("tall",) + synth.random_csr(4000, 2500, 4, seed=702, kind="empty_rows") + (2500,))  # rectangular, n < m, many empty rows
    return out


CASES = _build()  # (tag, rowptr, cols, vals, n)
TAGS = [c[0] for c in CASES]
# the reference's branch 1 (hip-adaptive/adaptive.cpp:34-35): halves that differ 4x or more in non-zeros
SPLIT_CASES = ("one", "one_long", "two_empty_first", "three", "odd_widths", "heavy_first", "straddle")
NOT_SPLIT_CASES = ("rpb_512", "rpb_513", "rpb_514", "wide", "tall", "tile_edges")
TRANS_CASE, TRANS_PAIR = "odd_widths", (2.0, 0.5)  # the driver's second pass, trans = 1


def case(tag):
    return CASES[TAGS.index(tag)]


def vectors(tag, m, n):
    """(x, y0) of a case: standard normal, from the case's own seed."""
    rng = np.random.default_rng(zlib.crc32(tag.encode()) ^ 0x5EED)
    return rng.standard_normal(n), rng.standard_normal(m)


def halves(rowptr):
    """(nnz of rows [0, m / 2), nnz of the rest): the true hints of the two hinted wrappers."""
    m = rowptr.size - 1
    return int(rowptr[m // 2]), int(rowptr[-1]) - int(rowptr[m // 2])


def hint_sets(rowptr):
    """The hint pairs adaptive_vec_row_sparse_spmv and adaptive_flat_sparse_spmv are called with.  They size lanes and workgroups only."""
    nnz = int(rowptr[-1])
    return [halves(rowptr), (0, 0), (nnz, 0), (0, nnz), (INT_MAX, 1)]


HINT_NAMES = ("true", "zero", "all_first", "all_second", "huge")

# the driver's calls on one (case, pair), in order.  adaptive_vec_row_sparse_spmv goes first on a fresh matrix (it makes no plan: the kernel query
# answers -2 after it) and once more at the end (it leaves the plan's record as the call before it left it)
CALLS = ([f"adaptive_vec_row[{h}]" for h in HINT_NAMES] +
         ["sparse_csr_spmv", "sparse_spmv", "default", "adaptive", "flat", "segment_sum_flat"] +
         [f"adaptive_flat[{h}]" for h in HINT_NAMES] +
         ["line_enhance", "adaptive_enhance", "adaptive_line", "line", "vec_row", "thread_row", "wf_row", "light", "block_row",
          "csr_adaptive_plus<true>", "csr_adaptive_plus<false>", "adaptive_vec_row[after]"])

MAGIC = 0x43585853


def write_input(path):
    """One file with all cases and pairs, as tests/cxx/surface_driver.cpp reads it: int32 {magic, cases, pairs, trans case, trans pair}, the pairs
    as doubles, then per case int32 {m, n, nnz}, rowptr, cols, vals, x, y0."""
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", MAGIC, len(CASES), len(ALPHA_BETA), TAGS.index(TRANS_CASE), ALPHA_BETA.index(TRANS_PAIR)))
        np.array(ALPHA_BETA, dtype=np.float64).tofile(f)
        for tag, rowptr, cols, vals, n in CASES:
            m = rowptr.size - 1
            x, y0 = vectors(tag, m, n)
            f.write(struct.pack("<3i", m, n, int(rowptr[-1])))
            for a, t in ((rowptr, np.int32), (cols, np.int32), (vals, np.float64), (x, np.float64), (y0, np.float64)):
                np.ascontiguousarray(a, dtype=t).tofile(f)


def read_output(path):
    """{(tag, pair index or 'trans', call): (y, error word, last kernel)} from the driver's output: per call m doubles, then the error word
    and the kernel query's answer as doubles; the main pass case by case and pair by pair, then the trans = 1 pass."""
    raw = np.fromfile(path, dtype=np.float64)
    out, pos = {}, 0
    runs = [(tag, k) for tag in TAGS for k in range(len(ALPHA_BETA))] + [(TRANS_CASE, "trans")]
    for tag, k in runs:
        m = case(tag)[1].size - 1
        for call in CALLS:
            rec = raw[pos:pos + m + 2]
            assert rec.size == m + 2, ("the driver's output ends early", tag, k, call)
            out[(tag, k, call)] = (rec[:m].copy(), int(rec[m]), int(rec[m + 1]))
            pos += m + 2
    assert pos == raw.size, ("the driver wrote more than the table asks for", pos, raw.size)
    return out


def hipcc_command(source, exe):
    """The line tests/test_gpu_parity.py::test_cxx_api_driver builds its driver with: the headers at the reference's include paths, libspmv_acc.so."""
    import os

    import spmv_acc_amd

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(spmv_acc_amd.LIB_PATH)
    return [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++14", "--offload-arch=gfx950", "-I", os.path.join(root, "include"),
            os.path.join(root, "tests", "cxx", source), "-L", libdir, "-lspmv_acc", f"-Wl,-rpath,{libdir}", "-o", str(exe)]
