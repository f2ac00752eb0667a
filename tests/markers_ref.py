"""The reference for --markers by the text of include/fastf_amd.h, by brute force: the doubled Mann-Whitney U of a label against every
other labelled cell as the double loop over the cells of a dense count array — no histogram, no floats — with det and sum beside it;
the ranking rule; the rows of markers.tsv.gz and <verb>_markers.tsv.  tables() is the definition in Python ints; tables_rows() is
the same double loop with the inner one over numpy int64 rows (exact: every term is below 2^33), for shapes the first cannot walk in
a test's time — test_markers_host holds the two against each other.  `wrong` names one deliberately wrong rule (the census)."""
import numpy as np

WRONG = ("ties_lost", "tie_to_higher_feature", "unlabelled_counted", "pairs_inside_counted")


def tables(counts, lab, n_labels, wrong=None):
    """counts: n x K (rows of Python ints); lab: per cell, 1 .. n_labels is labelled.  Returns (s2u, det, sum, n_per_label): three lists
    [a - 1][g] and one [a - 1]"""
    n, K = len(counts), (len(counts[0]) if len(counts) else 0)
    lab = [int(x) for x in lab]
    is_lab = [1 <= x <= n_labels for x in lab]
    s2u = [[0] * K for _ in range(n_labels)]
    det = [[0] * K for _ in range(n_labels)]
    tot = [[0] * K for _ in range(n_labels)]
    npl = [sum(1 for x in lab if x == a) for a in range(1, n_labels + 1)]
    for g in range(K):
        x = [int(counts[i][g]) for i in range(n)]
        for i in range(n):
            if not is_lab[i]:
                continue
            a = lab[i] - 1
            if x[i] > 0:
                det[a][g] += 1
                tot[a][g] += x[i]
            for j in range(n):
                if wrong == "unlabelled_counted":
                    if lab[j] == lab[i]:
                        continue
                elif wrong == "pairs_inside_counted":
                    if not is_lab[j]:
                        continue
                elif not is_lab[j] or lab[j] == lab[i]:
                    continue
                s2u[a][g] += 2 * (x[i] > x[j]) + (0 if wrong == "ties_lost" else (x[i] == x[j]))
    return s2u, det, tot, npl


def tables_rows(counts, lab, n_labels, columns=None):
    """tables() with the loop over j as one numpy row operation; columns: only these slots (the others are not computed: None there)"""
    x = np.asarray(counts, dtype=np.int64)
    n, K = x.shape
    lab = np.asarray(lab, dtype=np.int64)
    is_lab = (lab >= 1) & (lab <= n_labels)
    cols = list(range(K)) if columns is None else sorted(set(int(c) for c in columns))
    xs = x[:, cols]
    s2u = [[None] * K for _ in range(n_labels)]
    det = [[None] * K for _ in range(n_labels)]
    tot = [[None] * K for _ in range(n_labels)]
    npl = [int((lab == a).sum()) for a in range(1, n_labels + 1)]
    for a in range(1, n_labels + 1):
        ins, outs = xs[lab == a], xs[is_lab & (lab != a)]
        u = np.zeros(len(cols), np.int64)
        for row in ins:
            u += 2 * (row > outs).sum(axis=0) + (row == outs).sum(axis=0)
        d, t = (ins > 0).sum(axis=0), ins.sum(axis=0)
        for k, g in enumerate(cols):
            s2u[a - 1][g], det[a - 1][g], tot[a - 1][g] = int(u[k]), int(d[k]), int(t[k])
    return s2u, det, tot, npl


def ranks(s2u, npl, genes=None, wrong=None):
    """[a - 1][g]: the rank, from 1, of slot g for label a — descending 2U, ties by ascending feature number genes[g] (None: the slot);
    0 everywhere for a label with n_a == 0 or n_out == 0"""
    L, K = len(s2u), (len(s2u[0]) if s2u else 0)
    n_lab = sum(npl)
    sign = -1 if wrong == "tie_to_higher_feature" else 1
    out = []
    for a in range(L):
        if npl[a] == 0 or n_lab - npl[a] == 0:
            out.append([0] * K)
            continue
        order = sorted(range(K), key=lambda g: (-s2u[a][g], sign * (g if genes is None else int(genes[g]))))
        r = [0] * K
        for k, g in enumerate(order):
            r[g] = k + 1
        out.append(r)
    return out


def _f(num, den):
    return "%.6f" % (num / den)


POINT_HEADER = ["label", "gene", "rank_full", "rank_point", "auc_full", "auc_point", "det_in_full", "det_out_full", "det_in_point", "det_out_point",
                "mean_in_point"]
SUMMARY_TAIL = ["seed", "label", "n_in", "n_out", "top", "kept", "auc_full_mean", "auc_point_mean"]


def point_rows(names, gene_ids, top_n, full, point, rank_full, rank_point):
    """the rows of markers.tsv.gz behind the header.  names[0] == "NA"; gene_ids[g]: the feature id of slot g; full, point: tables()"""
    L, K = len(names) - 1, len(gene_ids)
    top = min(top_n, K)
    npl = full[3]
    n_lab = sum(npl)
    rows = []
    for a in range(L):
        n_in, n_out = npl[a], n_lab - npl[a]
        if n_in == 0 or n_out == 0:
            rows.append([names[a + 1]] + ["NA"] * 10)
            continue
        union = [g for g in range(K) if rank_full[a][g] <= top or rank_point[a][g] <= top]
        for g in sorted(union, key=lambda g: rank_full[a][g]):
            det_f, det_p = (sum(m[1][b][g] for b in range(L)) for m in (full, point))
            rows.append([names[a + 1], gene_ids[g], str(rank_full[a][g]), str(rank_point[a][g]), _f(full[0][a][g], 2 * n_in * n_out),
                         _f(point[0][a][g], 2 * n_in * n_out), str(full[1][a][g]), str(det_f - full[1][a][g]), str(point[1][a][g]),
                         str(det_p - point[1][a][g]), _f(point[2][a][g], n_in)])
    return rows


def summary_rows(lead, seed, names, K, top_n, full, point, rank_full, rank_point):
    """the n_labels + 1 rows of one point of <verb>_markers.tsv, as lists of fields"""
    L = len(names) - 1
    top = min(top_n, K)
    npl = full[3]
    n_lab = sum(npl)
    rows, all_out, all_top, all_kept, all_full, all_point = [], 0, 0, 0, 0.0, 0.0
    for a in range(L):
        n_in, n_out = npl[a], n_lab - npl[a]
        all_out += n_out
        head = list(lead) + [str(seed), names[a + 1], str(n_in), str(n_out), str(top)]
        if n_in == 0 or n_out == 0 or top == 0:
            rows.append(head + ["NA"] * 3)
            continue
        tops = [g for g in range(K) if 1 <= rank_full[a][g] <= top]
        kept = sum(1 for g in tops if 1 <= rank_point[a][g] <= top)
        den = 2.0 * n_in * n_out
        mf, mp = sum(full[0][a][g] for g in tops) / den, sum(point[0][a][g] for g in tops) / den
        all_top += top; all_kept += kept; all_full += mf; all_point += mp
        rows.append(head + [str(kept), "%.6f" % (mf / top), "%.6f" % (mp / top)])
    tail = ["%.6f" % (all_full / all_top), "%.6f" % (all_point / all_top)] if all_top else ["NA", "NA"]
    rows.append(list(lead) + [str(seed), "all", str(n_lab), str(all_out), str(all_top), str(all_kept)] + tail)
    return rows
