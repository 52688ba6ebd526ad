"""CPU suite of the C++ strategy surface: what tests/test_gpu_cxx_surface.py rests on, checked without a GPU.  The case table of
tests/cxx_surface_cases.py reaches the kernel forms it names (the reference's branch 1, the lane-width pairs, vector_row_kernel<1> / <4>, the
rows-per-workgroup boundary); tests/cxx/surface_driver.cpp compiles and links, and every one of the 19 C++-linkage entries it calls resolves in the
built library; adaptive_vec_row_sparse_spmv -- the one entry that launches without the engine -- refuses what the engine refuses, before it reaches the
HIP runtime."""
import subprocess

import numpy as np

import cxx_surface_cases as T
import spmv_acc_amd

K_THREADS, K_VEC_TILE_ROWS = 256, 2  # kernels.hpp kThreads; k_vector_row.hip kVecTileRows


def classic_vec(avg):  # config.cpp classic_vec: lanes per row that stream from global memory, 2 non-zeros per lane
    return next((w for w in (2, 4, 8, 16, 32) if avg <= 2 * w), 64)


def tile_vec(avg):  # config.cpp tile_vec: lanes per row over an LDS tile, 8 products per lane
    return next((w for w in (2, 4, 8, 16, 32) if 8 * w >= avg), 64)


def split_averages(rowptr):
    """The integer averages dispatch.cpp's split branch sizes its two widths from."""
    m = rowptr.size - 1
    half = m // 2
    first, second = T.halves(rowptr)
    return (first // half if half > 0 else 0), second // (m - half)


def test_the_table_holds_the_cases_of_its_docstring():
    shapes = {tag: (rowptr.size - 1, n, int(rowptr[-1])) for tag, rowptr, _, _, n in T.CASES}
    assert shapes["one"] == (1, 1, 1) and shapes["one_long"] == (1, 64, 5001) and shapes["two_empty_first"][::2] == (2, 300)
    assert shapes["three"] == (3, 4, 8)
    assert shapes["odd_widths"][::2] == (101, 50 + 51 * 40) and shapes["heavy_first"][::2] == (100, 30000)
    assert shapes["no_entries"] == (100, 5, 0) and shapes["straddle"] == (1500, 2000, 20000 + 4097 + 500)
    assert shapes["tile_edges"] == (40, 500, 40 * 1024)
    for m in (512, 513, 514):
        assert shapes[f"rpb_{m}"] == (m, m, 5 * m)
    assert shapes["wide"][:2] == (300, 900) and 80 * 300 <= shapes["wide"][2] <= 120 * 300
    assert shapes["tall"][:2] == (4000, 2500)
    assert set(T.SPLIT_CASES) | set(T.NOT_SPLIT_CASES) | {"no_entries"} == set(T.TAGS) and len(T.TAGS) == 14
    for tag, rowptr, cols, vals, n in T.CASES:
        m, nnz = rowptr.size - 1, int(rowptr[-1])
        assert rowptr.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.float64, tag
        assert rowptr[0] == 0 and np.all(np.diff(rowptr) >= 0) and cols.size == nnz == vals.size, tag
        assert nnz <= 50000 and (nnz == 0 or (cols.min() >= 0 and cols.max() < n)), tag  # small: a GPU test takes seconds
    # arrays whose length is no multiple of the 16-byte group of four (`three`, lengths [7, 0, 1], is not one of them: it holds 8)
    assert int(T.case("one_long")[1][-1]) % 4 == 1 and int(T.case("odd_widths")[1][-1]) % 4 == 2 and int(T.case("straddle")[1][-1]) % 4 == 1
    lens = np.diff(T.case("straddle")[1])
    assert lens[749] == 20000 and lens[750] == 4097 and np.all(lens[1400:] == 5) and lens.sum() == 24597
    assert np.array_equal(np.diff(T.case("three")[1]), [7, 0, 1]) and np.array_equal(np.diff(T.case("two_empty_first")[1]), [0, 300])
    assert T.ALPHA_BETA == [(1.0, 1.0), (-0.75, 0.0), (2.0, 0.5), (0.0, 1.5)]
    assert len(T.CALLS) == len(set(T.CALLS)) == 28


def test_split_cases_take_the_reference_branch_1(hiplib, oracle):
    """Branch 1 = halves that differ 4x or more: by the oracle's restatement of the reference's decision and by the library's own."""
    for tag in T.TAGS:
        rowptr = T.case(tag)[1]
        m = rowptr.size - 1
        want_split = tag in T.SPLIT_CASES
        picks = (oracle.adaptive_pick(rowptr), spmv_acc_amd.adaptive_branch(m, rowptr),
                 hiplib.spmv_acc_adaptive_branch(m, int(rowptr[m // 4]), int(rowptr[m // 2]), int(rowptr[3 * m // 4]), int(rowptr[m])))
        assert picks[0] == picks[1] == picks[2], (tag, picks)
        if tag != "no_entries":
            assert (picks[0] == 1) == want_split, (tag, picks)
    # the one case close to the limit: 20000 / 4597 is 4 in integer division, 20000 / 5001 would not be
    first, second = T.halves(T.case("straddle")[1])
    assert (first, second) == (20000, 4597) and first // second == 4 and 4 * second <= first < 5 * second


def test_split_cases_reach_the_width_pairs_they_are_named_for():
    """(w0, w1) of the split: tile form (vector_tile_kernel; also what adaptive_vec_row_sparse_spmv derives from the true hints) and classic form
    (vector_row_kernel)."""
    want = {"one": ((2, 2), (2, 2)), "one_long": ((2, 64), (2, 64)), "two_empty_first": ((2, 64), (2, 64)), "three": ((2, 2), (4, 2)),
            "odd_widths": ((2, 8), (2, 32)), "heavy_first": ((64, 2), (64, 2)), "straddle": ((4, 2), (16, 4))}
    assert set(want) == set(T.SPLIT_CASES)
    for tag, (tile, classic) in want.items():
        a0, a1 = split_averages(T.case(tag)[1])
        assert (tile_vec(a0), tile_vec(a1)) == tile, (tag, a0, a1)
        assert (classic_vec(a0), classic_vec(a1)) == classic, (tag, a0, a1)
    # the two rules against the thresholds config.cpp spells out
    assert [classic_vec(a) for a in (0, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64]
    assert [tile_vec(a) for a in (0, 16, 17, 32, 33, 64, 65, 256, 257, 10 ** 6)] == [2, 2, 4, 4, 8, 8, 16, 32, 64, 64]
    # the extreme pair in both orders, a pair of different widths below it, and equal widths
    pairs = {t for t, _ in want.values()} | {c for _, c in want.values()}
    assert {(2, 64), (64, 2), (2, 8), (2, 2)} <= pairs


def test_split_cases_reach_both_vector_row_instantiations():
    """launch_vector_row: one row per lane group (vector_row_kernel<1>) where nnz / m > 2 * max(w0, w1), four (vector_row_kernel<4>) otherwise."""
    got = {}
    for tag in T.SPLIT_CASES:
        rowptr = T.case(tag)[1]
        a0, a1 = split_averages(rowptr)
        got[tag] = 1 if int(rowptr[-1]) // (rowptr.size - 1) > 2 * max(classic_vec(a0), classic_vec(a1)) else 4
    assert got == {"one": 4, "one_long": 1, "two_empty_first": 1, "three": 4, "odd_widths": 4, "heavy_first": 1, "straddle": 4}


def test_rows_per_workgroup_boundary_and_tiles():
    """A width-2 workgroup of the tile form holds kVecTileRows * kThreads / 2 = 256 rows: the first halves of rpb_512 / _513 / _514 are 256, 256
    and 257 rows (one workgroup; one; two, the second with a single row), their second halves 256, 257, 257."""
    cap = K_VEC_TILE_ROWS * K_THREADS // 2
    assert cap == 256
    for m, half in ((512, 256), (513, 256), (514, 257)):
        rowptr = T.case(f"rpb_{m}")[1]
        assert m // 2 == half and split_averages(rowptr) == (5, 5) and tile_vec(5) == 2
        assert 1900 // 5 > cap  # (kVectorTarget products would ask for more rows than the cap: the cap decides)
    assert [-(-h // cap) for h in (256, 257)] == [1, 2]
    # rows longer than one 2048-product tile on both sides of m / 2, and rows that end exactly on tile boundaries
    lens = np.diff(T.case("straddle")[1])
    assert lens[1500 // 2 - 1] > 2048 and lens[1500 // 2] > 2048 and lens[1500 // 2] % 2048 == 1
    assert np.all(T.case("tile_edges")[1][1:] % 1024 == 0) and np.all(T.case("tile_edges")[1][2::2] % 2048 == 0)


def test_input_file_round_trip(tmp_path):
    """What write_input writes is what the driver's reader expects: the header, then every case at the offset its sizes give."""
    path = tmp_path / "cases.bin"
    T.write_input(path)
    raw = path.read_bytes()
    hdr = np.frombuffer(raw, dtype=np.int32, count=5)
    assert hdr.tolist() == [T.MAGIC, 14, 4, T.TAGS.index("odd_widths"), 2]
    pos = 20 + 16 * 4
    for tag, rowptr, cols, vals, n in T.CASES:
        m, nnz = rowptr.size - 1, int(rowptr[-1])
        assert np.frombuffer(raw, dtype=np.int32, count=3, offset=pos).tolist() == [m, n, nnz], tag
        assert np.array_equal(np.frombuffer(raw, dtype=np.int32, count=m + 1, offset=pos + 12), rowptr), tag
        pos += 12 + 4 * (m + 1) + 12 * nnz + 8 * (n + m)
    assert pos == len(raw)


# the 19 C++-linkage entries (include/api/spmv.h, include/spmv_acc_strategies.hpp), as `nm -C` prints the start of each
SURFACE = ["sparse_csr_spmv(int, double, double, csr_desc<int, double>, csr_desc<int, double>",
           "sparse_spmv(int, double, double, int, int, int const*", "default_sparse_spmv(", "adaptive_sparse_spmv(", "flat_sparse_spmv(",
           "segment_sum_flat_sparse_spmv(", "adaptive_flat_sparse_spmv(", "line_enhance_sparse_spmv(", "adaptive_enhance_sparse_spmv(",
           "adaptive_line_sparse_spmv(", "line_sparse_spmv(", "vec_row_sparse_spmv(", "adaptive_vec_row_sparse_spmv(", "thread_row_sparse_spmv(",
           "wf_row_sparse_spmv(", "light_sparse_spmv(", "block_row_sparse_spmv(",
           "void csr_adaptive_plus_sparse_spmv<true, int, double>(SpMVAccHanele*",
           "void csr_adaptive_plus_sparse_spmv<false, int, double>(SpMVAccHanele*"]


def _symbols(args):
    out = subprocess.run(["nm", "-C"] + args, capture_output=True, text=True, check=True).stdout
    return [line.split(None, 2 if line[:1] not in " \t" else 1)[-1].strip() for line in out.splitlines() if line.strip()]


def test_surface_driver_links_and_every_entry_resolves(hiplib, tmp_path):
    """tests/cxx/surface_driver.cpp compiles against the headers at the reference's include paths and links libspmv_acc.so; each of the 19 entries
    is an undefined symbol of the program that the library defines under exactly that (demangled) signature."""
    exe = tmp_path / "surface_driver"
    subprocess.run(T.hipcc_command("surface_driver.cpp", exe), check=True)
    wanted = _symbols(["-u", str(exe)])
    defined = set(_symbols(["-D", "--defined-only", spmv_acc_amd.LIB_PATH]))
    assert len(SURFACE) == 19
    for name in SURFACE:
        hits = [s for s in wanted if s.startswith(name)]
        assert len(hits) == 1, (name, hits)
        assert hits[0] in defined, hits[0]
    # the C++-linkage sparse_spmv, not its C twin of the same name
    assert "sparse_spmv" not in wanted
    # no file: the program ends before it touches a device
    assert subprocess.run([str(exe)], capture_output=True, timeout=60).returncode == 2


def test_adaptive_vec_row_refuses_bad_arguments_without_a_gpu(hiplib, tmp_path):
    """tests/cxx/surface_refusals.cpp: null rowptr / y / x (n > 0) / colindex (nnz > 0) are SPMV_ACC_ERR_BAD_ARGUMENT, m > INT_MAX - 65536 is
    SPMV_ACC_ERR_TOO_LARGE, trans != 0 is reported even where there is nothing to compute, m == 0 is no error -- the engine's answers
    (dispatch.cpp spmv_call_accepted), given before anything reaches the HIP runtime: the program runs on a machine without a GPU."""
    exe = tmp_path / "surface_refusals"
    subprocess.run(T.hipcc_command("surface_refusals.cpp", exe), check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    got = dict(line.split() for line in r.stdout.splitlines())
    bad, too_large, trans = str(2), str(4), str(1)  # include/spmv_acc.h enum spmv_acc_error
    assert got == {"null_rowptr": bad, "null_y": bad, "null_x": bad, "null_colindex": bad, "too_many_rows": too_large,
                   "trans_without_rows": trans, "no_rows": "0"}, r.stdout
