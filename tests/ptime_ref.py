"""--pseudotime by its definition (include/fastf_amd.h) in Python ints and floats: the rules of the file, the doubled midranks, the lower
median by sorting, the census by the double loop over all pairs, and the two printed ratios in the operation order the header states.
Nothing here is shared with the code under test."""
import math
import re

OUT_WORDS = 7       # conc disc tie_e tie_t tie_both cells shift_sum
VALUE_BYTES = 63

# what strtod accepts in the C locale, the whole string: blanks in front, a sign, then a decimal or a hexadecimal number, inf or nan
_NUMBER = re.compile(r"^[ \t\n\v\f\r]*[+-]?(?:(?P<hex>0[xX](?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)(?:[pP][+-]?[0-9]+)?)"
                     r"|(?P<dec>(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)"
                     r"|(?P<inf>[iI][nN][fF](?:[iI][nN][iI][tT][yY])?)|(?P<nan>[nN][aA][nN](?:\([0-9a-zA-Z_]*\))?))$")


class Refused(Exception):
    """the file is refused: .line is the line number (0: the file as a whole), .why a word for the rule"""

    def __init__(self, why, line=0):
        Exception.__init__(self, "%s (line %d)" % (why, line))
        self.why, self.line = why, line


def parse_value(text):
    """None for NA, else the float; Refused("number") / Refused("finite") without a line"""
    if text == "NA":
        return None
    m = _NUMBER.match(text)
    if not m:
        raise Refused("number")
    if m.group("inf") or m.group("nan"):
        raise Refused("finite")
    try:
        v = float.fromhex(text.strip()) if m.group("hex") else float(text.strip())
    except OverflowError:
        v = math.inf
    if math.isinf(v):
        raise Refused("finite")
    return v


def parse_file(data, listed):
    """data: the bytes of the file; listed: the barcodes of the barcode list.  Returns (values, known, unknown): values maps every
    LISTED barcode that has a line to its float or None (NA); known / unknown count the lines whose barcode is / is not listed"""
    if data[:2] == b"\x1f\x8b":
        raise Refused("gzip")
    values, seen, known, unknown = {}, {}, 0, 0
    listed = set(listed)
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    dup = None
    for no, raw in enumerate(lines, 1):
        if raw.endswith(b"\r"):
            raw = raw[:-1]
        if not raw:
            continue
        if b"\0" in raw:
            raise Refused("nul", no)
        fields = raw.split(b"\t")
        if len(fields) != 2:
            raise Refused("fields", no)
        barcode, value = fields[0].decode("latin-1"), fields[1].decode("latin-1")
        if no == 1 and barcode == "barcode":
            continue
        if not value:
            raise Refused("empty", no)
        if len(value) > VALUE_BYTES:
            raise Refused("long", no)
        try:
            v = parse_value(value)
        except Refused as r:
            raise Refused(r.why, no)
        if barcode in seen:
            dup = dup or no                                 # (the first line that names a barcode again; the lines before it were read whole)
            continue
        seen[barcode] = no
        if barcode in listed:
            known += 1
            values[barcode] = v
        else:
            unknown += 1
    if dup:
        raise Refused("twice", dup)
    if not known:
        raise Refused("none")
    return values, known, unknown


def midranks(values):
    """values: one float or None per cell -> (t, m): t[i] = 2 #{v_j < v_i} + #{v_j == v_i} + 1 over the m valued cells, 0 without a value"""
    have = [v for v in values if v is not None]
    t = [0 if v is None else 2 * sum(1 for w in have if w < v) + sum(1 for w in have if w == v) + 1 for v in values]
    return t, len(have)


def medians(lists, t):
    """lists[i]: the neighbours of cell i (indices below len(t) only) -> (est, valued): the lower median of their non-zero t, their number"""
    est, valued = [], []
    for nb in lists:
        v = sorted(t[j] for j in nb if t[j] > 0)
        valued.append(len(v))
        est.append(v[(len(v) + 1) // 2 - 1] if v else 0)
    return est, valued


def census(est, t):
    """[conc, disc, tie_e, tie_t, tie_both, cells, shift_sum] over the cells with t > 0 and est > 0, pair by pair"""
    s = [i for i in range(len(t)) if t[i] > 0 and est[i] > 0]
    c = [0] * OUT_WORDS
    for a, i in enumerate(s):
        for j in s[a + 1:]:
            p = (est[i] - est[j]) * (t[i] - t[j])
            if p > 0:
                c[0] += 1
            elif p < 0:
                c[1] += 1
            elif est[i] == est[j] and t[i] != t[j]:
                c[2] += 1
            elif t[i] == t[j] and est[i] != est[j]:
                c[3] += 1
            else:
                c[4] += 1
    c[5] = len(s)
    c[6] = sum(abs(est[i] - t[i]) for i in s)
    return c


def tau_text(c):
    conc, disc, tie_e, tie_t = c[:4]
    if conc + disc + tie_e == 0 or conc + disc + tie_t == 0:
        return "NA"
    return "%.6f" % (float(conc - disc) / math.sqrt(float(conc + disc + tie_e) * float(conc + disc + tie_t)))


def shift_text(c, m):
    if m == 0 or c[5] == 0:
        return "NA"
    return "%.6f" % (float(c[6]) / (float(2 * m) * float(c[5])))


def census_fields(c, m):
    return ["NA"] * 5 if c is None else [str(c[5]), str(c[0]), str(c[1]), tau_text(c), shift_text(c, m)]


def summary_fields(lead, seed, n_cells, k, m, c_full, c_point, c_map=None):
    """the fields of one row of <verb>_pseudotime.tsv; lead: the verb's two leading columns as text"""
    return list(lead) + [str(seed), str(n_cells), str(k), str(m)] + census_fields(c_full, m) + census_fields(c_point, m) + census_fields(c_map, m)


def _na(v):
    return str(v) if v else "NA"


def cell_rows(barcodes, t, full, point, mapped=None):
    """the rows of pseudotime.tsv.gz as lists of fields; full, point, mapped: (est, valued)"""
    return [[bc, _na(t[i]), _na(full[0][i]), str(full[1][i]), _na(point[0][i]), str(point[1][i])] +
            ([_na(mapped[0][i]), str(mapped[1][i])] if mapped else ["NA", "NA"]) for i, bc in enumerate(barcodes)]
