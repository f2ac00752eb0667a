"""The reference for --labels in plain Python on index lists, by the text of include/fastf_amd.h: the votes of a cell's neighbours for
the labels 1 .. L, pred (most votes, ties to the smallest label, 0 without a labelled neighbour), same, labelled, the confusion
counts, and the rows of labels.tsv.gz, label_confusion.tsv.gz, <verb>_labels.tsv and <verb>_label_classes.tsv.  The neighbour sets
come from neighbors_ref."""
import numpy as np

import neighbors_ref as N

NONE = N.NONE


def votes(sets, lab, n_labels):
    """sets: per cell the list of its neighbours (0-based); lab: per cell 0 .. n_labels.  Returns (pred, same, labelled, conf) with
    conf[a - 1][b] for a in 1 .. L, b in 0 .. L"""
    pred, same, labelled = [], [], []
    conf = [[0] * (n_labels + 1) for _ in range(n_labels)]
    for i, nb in enumerate(sets):
        v = [0] * (n_labels + 1)
        for j in nb:
            if 1 <= lab[j] <= n_labels:
                v[lab[j]] += 1
        total = sum(v)
        p = 0 if total == 0 else min(range(1, n_labels + 1), key=lambda l: (-v[l], l))
        pred.append(p); labelled.append(total); same.append(v[lab[i]] if lab[i] else 0)
        if lab[i]:
            conf[lab[i] - 1][p] += 1
    return pred, same, labelled, conf


def sets_of_slots(idx, cnt):
    """the lists of a slot array (n x k) and its counts: the slots from cnt[i] on are not read"""
    return [[int(v) for v in row[:c]] for row, c in zip(np.asarray(idx), np.asarray(cnt))]


def _ratio(a, b):
    return "NA" if b == 0 else "%.6f" % (a / b)


def cell_rows(barcodes, names, lab, full, point):
    """full, point: (pred, same, labelled, conf)"""
    return [[bc, names[lab[i]], names[full[0][i]], names[point[0][i]], str(full[1][i]), str(full[2][i]), str(point[1][i]), str(point[2][i])]
            for i, bc in enumerate(barcodes)]


def confusion_rows(names, lab, conf):
    L = len(names) - 1
    return [["label", "cells", "NA"] + names[1:]] + [[names[a], str(sum(1 for x in lab if x == a))] + [str(v) for v in conf[a - 1]] for a in range(1, L + 1)]


def summary_fields(lead, seed, k, n_labels, lab, full, point):
    ids = [i for i, x in enumerate(lab) if x >= 1]
    agree = [sum(c[a][a + 1] for a in range(n_labels)) for c in (full[3], point[3])]
    kept = sum(1 for i in ids if full[0][i] == lab[i] and point[0][i] == lab[i])
    pur = [_ratio(sum(m[1][i] for i in ids), sum(m[2][i] for i in ids)) for m in (full, point)]
    return list(lead) + [str(seed), str(len(lab)), str(k), str(n_labels), str(len(ids)), str(agree[0]), str(agree[1]), _ratio(agree[0], len(ids)),
                         _ratio(agree[1], len(ids)), _ratio(kept, agree[0])] + pur


def classes_fields(lead, seed, names, lab, full, point):
    L = len(names) - 1
    return [list(lead) + [str(seed), names[a], str(sum(1 for x in lab if x == a)), str(full[3][a - 1][a]), str(point[3][a - 1][a]),
                          str(sum(full[3][r][a] for r in range(L))), str(sum(point[3][r][a] for r in range(L)))] for a in range(1, L + 1)]


def label_ids(pairs):
    """pairs: (barcode, label) of a file.  Returns (names with "NA" first, {barcode: id})"""
    names = ["NA"] + sorted({l for _, l in pairs if l != "NA"}, key=lambda s: s.encode())
    return names, {b: (0 if l == "NA" else names.index(l)) for b, l in pairs}
