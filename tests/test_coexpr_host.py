"""Co-expression partners on the host: the host twin (fastf_coexpr_from_coo, fastf_coexpr_select) against coexpr_ref on hand-built and
random matrices — ties at the cut, products beyond 128 bits, zero and negative covariance, genes without variance, rows in any order —
the range rule on both sides of 2^63, the bound of the sums of products, the rows and headers, and the exported names."""
import numpy as np
import pytest

import fastf_amd as F
from fastf_amd import _lib, cap, level, sweep
import coexpr_ref as R


def as_lists(idx, cnt):
    return [[int(v) for v in idx[g, :cnt[g]]] for g in range(len(cnt))]


def twin(rows, n, nf, genes, k):
    idx, cnt, D, S = sweep.coexpression_from_coo(rows, n, R.slot_map(genes, nf), len(genes), k)
    assert all((idx[g, cnt[g]:] == 0xFFFFFFFF).all() for g in range(len(genes)))
    return as_lists(idx, cnt), [[int(v) for v in row] for row in D], [int(v) for v in S]


def test_the_census_of_the_fixtures():
    c = R.census()
    assert "wide" in c["wide_changes_a_set"]
    assert "duplicates" in c["tie_by_slot"] and "proportional" in c["tie_by_slot"] and c["float_differs"] == ["proportional"]
    assert "zero_cov" in c["zero_cov"] and "negative" in c["negative_cov"] and "degenerate" in c["zero_variance"]
    # the named cases are what they are called
    assert R.reference("duplicates")[2][0] == [1, 2]                        # slots 2 and 3 are one column: the lower one stays
    assert R.reference("proportional")[2][0] == [1]                         # slot 2 = 3 x slot 1: the tie goes to slot 1
    assert R.reference("zero_cov")[2][:2] == [[2], [2]]                      # c_01 == 0: 0 and 1 are no partners
    assert R.reference("negative")[2][1] == []                              # slot 1 runs against both others
    D, S, sets = R.reference("degenerate")
    assert sets[0] == [] and sets[1] == [] and all(0 not in s and 1 not in s for s in sets)
    assert R.reference("one_gene")[2] == [[]] and R.reference("one_cell")[2] == [[], [], []]
    assert max(len(s) for s in R.reference("few_candidates")[2]) < 15
    assert {R.FIXTURES[n][4] for n in ("k1", "k15", "k64")} == {1, 15, 64}


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_host_twin_against_the_reference(name):
    rows, n, nf, genes, k = R.FIXTURES[name]
    D, S, sets = R.reference(name)
    got, gD, gS = twin(rows, n, nf, genes, k)
    assert gD == D and gS == S
    assert got == sets
    order = np.random.default_rng(5).permutation(len(rows[0]))              # rows in any order
    assert twin(tuple(a[order] for a in rows), n, nf, genes, k)[0] == sets
    idx, cnt = sweep.coexpression_select(np.array(D, np.uint64).reshape(len(S), len(S)), np.array(S, np.uint64), n, k)
    assert as_lists(idx, cnt) == sets


@pytest.mark.parametrize("name", ["k15", "wide", "duplicates"])
def test_other_k_on_the_same_matrix(name):
    rows, n, nf, genes, _ = R.FIXTURES[name]
    D, S, _ = R.reference(name)
    for k in (1, 2, 15, 64):
        assert twin(rows, n, nf, genes, k)[0] == R.partner_sets(D, S, n, k)


def test_a_128_bit_compare_would_fail_the_wide_fixture():
    rows, n, nf, genes, k = R.FIXTURES["wide"]
    D, S, sets = R.reference("wide")
    assert R.partner_sets(D, S, n, k, 128) != sets and twin(rows, n, nf, genes, k)[0] == sets


def test_range_rule_on_both_sides_of_2_63():
    sweep.coexpression_check_range(1, (1 << 63) - 1)
    sweep.coexpression_check_range(1 << 20, (1 << 43) - 1)
    sweep.coexpression_check_range(0, (1 << 64) - 1)
    for n, q in ((1, 1 << 63), (1 << 20, 1 << 43), (3, ((1 << 63) + 2) // 3), ((1 << 32) - 1, 1 << 32)):
        assert n * q >= 1 << 63
        with pytest.raises(F.FastfError, match="FASTF_ERR_COEXPR_RANGE"):
            sweep.coexpression_check_range(n, q)
    sweep.coexpression_check_range(3, ((1 << 63) - 1) // 3)
    # through the twin: one gene with v in every one of n cells: n * n * v^2 against 2^63
    for v, n, ok in (((1 << 21) - 1, 1448, True), ((1 << 21) - 1, 1449, False)):
        assert (n * n * v * v < 1 << 63) == ok
        rows = (np.full(n, 1, np.uint32), np.arange(1, n + 1, dtype=np.uint32), np.full(n, v, np.uint32))
        if ok:
            assert twin(rows, n, 1, [0], 15)[1] == [[n * v * v]]
        else:
            with pytest.raises(F.FastfError, match="FASTF_ERR_COEXPR_RANGE"):
                twin(rows, n, 1, [0], 15)


def test_refusals_of_the_twin():
    rows, n, nf, genes, k = R.FIXTURES["k15"]
    for bad_k in (0, 65):
        with pytest.raises(F.FastfError, match="from 1 to 64"):
            twin(rows, n, nf, genes, bad_k)
    big = (rows[0], rows[1], np.where(np.arange(len(rows[2])) == 0, 1 << 21, rows[2]).astype(np.uint32))
    with pytest.raises(F.FastfError, match="FASTF_ERR_NEIGHBOR_COUNT"):
        twin(big, n, nf, genes, k)
    L = _lib.lib()
    assert L.fastf_coexpr_check_gram(1 << 22, 3) == 0 and L.fastf_coexpr_check_gram((1 << 32) - 1, 2) == 0
    assert L.fastf_coexpr_check_gram((1 << 22) + 5, 3) == 1 and "FASTF_ERR_COEXPR_CELLS" in L.fastf_last_error().decode()
    assert L.fastf_coexpr_check_gram(5, 0) == 1 and L.fastf_coexpr_check_gram(5, 4) == 1


def test_rows_headers_and_na_rules():
    assert sweep.coexpression_header() == "\t".join(sweep.POINT_COEXPRESSION_COLUMNS) + "\n"
    assert sweep.coexpression_header("sweep") == "\t".join(sweep.COEXPRESSION_COLUMNS) + "\n"
    assert sweep.coexpression_header("cap").split("\t")[:2] == list(cap.NEIGHBORS_COLUMNS[:2])
    assert sweep.coexpression_header("level").split("\t")[:2] == list(level.NEIGHBORS_COLUMNS[:2])
    assert sweep.coexpression_header("cap").split("\t")[2:] == sweep.coexpression_header("sweep").split("\t")[2:] == sweep.coexpression_header("level").split("\t")[2:]
    assert sweep.coexpression_row("ENSG01", 15, 14, 9) == "ENSG01\t15\t14\t9\n"
    kf, kp, sh = [15, 0, 3, 2, 1], [15, 2, 0, 2, 1], [15, 0, 0, 1, 0]
    want = R.summary_fields(["0.500", "0.250"], 926, 77, 15, kf, kp, sh)
    got = sweep.coexpression_summary_row(0.5, 0.25, 926, 77, kf, kp, sh).rstrip("\n").split("\t")
    assert got[:10] == want[:10] and got[11] == want[11] == "2" and abs(float(got[10]) - float(want[10])) <= 5e-7
    assert got[6:10] == ["4", "21", "20", "16"]
    row = sweep.coexpression_summary_row(0.5, 0, 4, 9, [0, 0], [3, 0], [0, 0], list_value=250, k=7).rstrip("\n").split("\t")
    assert row == ["0.500", "250", "4", "9", "2", "7", "0", "0", "3", "0", "NA", "0"]
    assert sweep.coexpression_summary_row(1, 1, 1, 0, [], [], []).rstrip("\n").split("\t")[4:] == ["0", "15", "0", "0", "0", "0", "NA", "0"]


def test_exported_names():
    L = _lib.lib()
    for name in ("fastf_coexpr_header", "fastf_sweep_coexpr_header", "fastf_cap_coexpr_header", "fastf_level_coexpr_header", "fastf_coexpr_check_range",
                 "fastf_coexpr_check_gram", "fastf_coexpr_row", "fastf_coexpr_summary_row", "fastf_coexpr_from_coo", "fastf_coexpr_select"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
