/* diagnostic: the tables and point files of a grid run (fastf_amd/csrc/res_tables.c) on the CPU, under sanitizers.  The host views of a
 * res_rate_t are filled by hand — every array a malloc of exactly the entries the writers may read — and open, point and close are
 * driven in a temporary directory; no engine, no device pointer.  What is checked, for n_cells in {0, 1, 5} x n_features in {0, 1, 4}
 * x 1 and 3 labels, --markers N below and above hvg_k = min(2, n_features) (2: the smallest K with an N on either side), the three
 * verbs in turn:
 *   point files   every comparison, --genes and --cells on, two points: each <verb>_*.tsv is its header plus the rows the public
 *                 *_summary_row functions give for the same arrays, each point file gunzips to its header plus the public *_row lines
 *                 (markers.tsv.gz: the selection written out again below), no .partial is left
 *   summary only  the same with dir == NULL: the same tables and no point directory
 *   failed run    close with ok == 0 leaves nothing
 *   failed rename a non-empty directory at <out>/<verb>_neighbors.tsv: close returns 1, the message names that file, no table and no
 *                 .partial is left
 *   subsets       each comparison alone, and labels without markers, open their own files only
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ifastf_amd/csrc -Itools tools/res_tables_check.c fastf_amd/csrc/{res_tables,grid_rows,host_io,host_prims,inflate_fast,crc32_fast,deflate_fast}.c -lz -lpthread -lm -o build/res_tables_check
 *   build/res_tables_check <empty dir>   -> "tables hold: <n> runs" */
#define _GNU_SOURCE
#define SAN_KEEP_ERROR
#include "fastf_amd.h"
#include "resident.h"
#include "san_stubs.h"
#include "../fastf_amd/csrc/coexpr_host.c"       /* the rows of --coexpression live in coexpr_host.c; tests/test_sanitizers.py::test_grid_tables_and_point_files_hold_on_hand_filled_views compiles this program with res_tables.c, grid_rows.c and the host_io sources only, so the file is compiled in here and the gcc line of the comment above needs no coexpr_host.c */
#include <dirent.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (%s) [%s]\n", __FILE__, __LINE__, #c, g_case, fastf_last_error()); exit(1); } } while (0)
static char g_case[160];
static const char *(*const summary_header[3])(void) = { fastf_sweep_header, fastf_cap_header, fastf_level_header };
static const char *const verb_name[3] = { "sweep", "cap", "level" };
const char *fastf_cap_header(void) { return "cap\n"; }       /* (cap_cmds.c is device code: only <verb>.tsv would need them) */
const char *fastf_level_header(void) { return "level\n"; }

/* ---- files ---- */
static char *slurp(const char *path, int gz)
{
    size_t len = 0, cap = 1 << 16;
    char *p = (char *)malloc(cap);
    gzFile g = gzopen(path, "rb");           /* (reads a plain file as it is) */
    CHECK(g && p);
    CHECK(!gz || !gzdirect(g));
    for (int n; (n = gzread(g, p + len, (unsigned)(cap - len - 1))) > 0;) { len += (size_t)n; if (len + 1 == cap) CHECK((p = (char *)realloc(p, cap *= 2))); }
    gzclose(g);
    p[len] = '\0';
    return p;
}
static void expect_file(const char *dir, const char *name, const char *want, int gz)
{
    char path[4400];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    char *got = slurp(path, gz);
    if (strcmp(got, want)) { fprintf(stderr, "%s (%s):\n--- got\n%s--- want\n%s", path, g_case, got, want); exit(1); }
    free(got);
}
static int cmp_str(const void *a, const void *b) { return strcmp((const char *)a, (const char *)b); }
/* n names, sorted, joined by blanks */
typedef char name_t[96];
static void joined(name_t *names, int n, char *out)
{
    qsort(names, (size_t)n, sizeof *names, cmp_str);
    out[0] = '\0';
    for (int i = 0; i < n; i++) { strcat(out, i ? " " : ""); strcat(out, names[i]); }
}
/* the entries of dir */
static const char *listing(const char *dir)
{
    static char out[4096];
    name_t names[32];
    int n = 0;
    DIR *d = opendir(dir);
    CHECK(d);
    for (struct dirent *e; (e = readdir(d));) if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) { CHECK(n < 32 && strlen(e->d_name) < sizeof *names); strcpy(names[n++], e->d_name); }
    closedir(d);
    joined(names, n, out);
    return out;
}
static void remove_tree(const char *dir)
{
    DIR *d = opendir(dir);
    if (!d) { unlink(dir); return; }
    for (struct dirent *e; (e = readdir(d));) {
        char path[4400];
        if (!strcmp(e->d_name, ".") || !strcmp(e->d_name, "..")) continue;
        snprintf(path, sizeof path, "%s/%s", dir, e->d_name);
        remove_tree(path);
    }
    closedir(d);
    rmdir(dir);
}

/* ---- one pair state, by hand ---- */
typedef struct { res_rate_t S; fastf_lists_t L; fastf_labels_t *labels; void *own[64]; int n_own; } state_t;
static void *own(state_t *st, size_t n, size_t elem) { void *p = malloc(n ? n * elem : 1); CHECK(p && st->n_own < 64); memset(p, 0, n * elem); return st->own[st->n_own++] = p; }
#define OWN(st, field, n) ((field) = own((st), (n), sizeof *(field)))

static void state_make(state_t *st, const char *tmp, uint32_t nc, uint32_t nf, uint32_t n_labels)
{
    static const char *const label_of[5] = { "T", "B", "NK", "T", "B" };
    res_rate_t *S = &st->S;
    char bpath[4400], lpath[4400];
    memset(st, 0, sizeof *st);
    /* the labels: five barcodes of a list of their own — the tables take the names from it and nothing else */
    snprintf(bpath, sizeof bpath, "%s/barcodes.tsv", tmp); snprintf(lpath, sizeof lpath, "%s/labels.tsv", tmp);
    FILE *b = fopen(bpath, "w"), *l = fopen(lpath, "w");
    CHECK(b && l);
    for (int i = 0; i < 5; i++) { fprintf(b, "BC%d\n", i); fprintf(l, "BC%d\t%s\n", i, n_labels == 1 ? "T" : label_of[i]); }
    fclose(b); fclose(l);
    CHECK(!fastf_labels_load(lpath, bpath, &st->labels) && fastf_labels_count(st->labels) == n_labels);
    unlink(bpath); unlink(lpath);

    const uint32_t K = nf < 2 ? nf : 2, L = n_labels;
    S->L = &st->L; S->rate_cell = 0.5f; S->seed = 926; S->n_cells = nc; S->n_features = nf; S->hvg_k = K; S->n_labels = L;
    st->L.n_cells = nc; st->L.n_features = nf;
    OWN(st, st->L.barcode, nc); OWN(st, st->L.feat_id, nf);
    for (uint32_t c = 0; c < nc; c++) { OWN(st, st->L.barcode[c], 24); snprintf(st->L.barcode[c], 24, "CELL%u-1", c); }
    for (uint32_t g = 0; g < nf; g++) { OWN(st, st->L.feat_id[g], 16); snprintf(st->L.feat_id[g], 16, "GENE%u", g); }
    /* the counts of a full matrix X and of a point Y = X / 2, and every sum of them the comparisons read */
    OWN(st, S->buf.h_upc.u64, nc + 1); OWN(st, S->buf.h_gpc.u32, nc); OWN(st, S->buf.h_cpg.u32, nf); OWN(st, S->buf.h_upg.u64, nf);
    OWN(st, S->h_fid.ufull, nc + 1); OWN(st, S->h_fid.gfull, nc); OWN(st, S->h_fid.sxx, nc); OWN(st, S->h_fid.syy, nc); OWN(st, S->h_fid.sxy, nc);
    OWN(st, S->h_gfid.sx, nf); OWN(st, S->h_gfid.sxx, nf); OWN(st, S->h_gfid.sy, nf); OWN(st, S->h_gfid.syy, nf); OWN(st, S->h_gfid.sxy, nf); OWN(st, S->h_gfid.cf, nf); OWN(st, S->h_gfid.c, nf);
    for (uint32_t c = 0; c < nc; c++) for (uint32_t g = 0; g < nf; g++) {
        const uint64_t x = (c * 7 + g * 3 + 1) % 6, y = x / 2;
        S->h_fid.ufull[c] += x; S->h_fid.gfull[c] += x > 0; S->h_fid.sxx[c] += x * x; S->h_fid.syy[c] += y * y; S->h_fid.sxy[c] += x * y;
        S->buf.h_upc.u64[c] += y; S->buf.h_gpc.u32[c] += y > 0; S->buf.h_upc.u64[nc] += y; S->h_fid.ufull[nc] += x;
        S->h_gfid.sx[g] += x; S->h_gfid.sxx[g] += x * x; S->h_gfid.sy[g] += y; S->h_gfid.syy[g] += y * y; S->h_gfid.sxy[g] += x * y; S->h_gfid.cf[g] += x > 0; S->h_gfid.c[g] += y > 0;
        S->buf.h_cpg.u32[g] += y > 0; S->buf.h_upg.u64[g] += y;
    }
    /* --cells */
    OWN(st, S->h_cs.hist, FASTF_COPY_BINS + 1); OWN(st, S->h_cs.rpc, nc); OWN(st, S->h_cs.npc, nc); OWN(st, S->h_cs.spc, nc);
    for (uint32_t c = 0; c < nc; c++) { S->h_cs.rpc[c] = (uint32_t)S->buf.h_upc.u64[c] * 2 + c; S->h_cs.npc[c] = c & 1; S->h_cs.spc[c] = c; S->h_cs.hist[c % 3] += S->buf.h_upc.u64[c]; }
    /* --neighbors: the genes of A are the last K features */
    OWN(st, S->h_nbr.kf, nc); OWN(st, S->h_nbr.kp, nc); OWN(st, S->h_nbr.sh, nc); OWN(st, S->h_nbr.genes, K);
    for (uint32_t c = 0; c < nc; c++) { S->h_nbr.kf[c] = nc - 1; S->h_nbr.kp[c] = c ? nc - 2 : 0; S->h_nbr.sh[c] = c / 2; }
    for (uint32_t g = 0; g < K; g++) S->h_nbr.genes[g] = nf - 1 - g;
    /* --coexpression: per gene of A (its own copy of the genes: the option runs without --neighbors) */
    OWN(st, S->h_cx.kf, K); OWN(st, S->h_cx.kp, K); OWN(st, S->h_cx.sh, K); OWN(st, S->h_cx.genes, K);
    for (uint32_t g = 0; g < K; g++) { S->h_cx.genes[g] = nf - 1 - g; S->h_cx.kf[g] = K - 1; S->h_cx.kp[g] = g ? K - 1 : 0; S->h_cx.sh[g] = g; }
    /* --labels */
    OWN(st, S->h_lab.lab, nc);
    for (int h = 0; h < 2; h++) { OWN(st, S->h_lab.half[h].pred, nc); OWN(st, S->h_lab.half[h].same, nc); OWN(st, S->h_lab.half[h].labelled, nc); OWN(st, S->h_lab.half[h].conf, (size_t)L * (L + 1)); }
    for (uint32_t c = 0; c < nc; c++) {
        const uint8_t a = S->h_lab.lab[c] = (uint8_t)(c % (L + 1));
        for (int h = 0; h < 2; h++) {
            const uint8_t p = S->h_lab.half[h].pred[c] = (uint8_t)((c + (uint32_t)h) % (L + 1));
            S->h_lab.half[h].labelled[c] = (uint8_t)(nc - 1); S->h_lab.half[h].same[c] = (uint8_t)(c % nc / 2);
            if (a) S->h_lab.half[h].conf[(size_t)(a - 1) * (L + 1) + p]++;
        }
    }
    /* --markers: two sets of tables of exactly L x K entries, the ranks a permutation per label (the point's: the full ones reversed) */
    S->mk_set = res_mk_set_bytes(L, K);
    OWN(st, S->buf.h_mk.u8, 2 * S->mk_set); OWN(st, S->buf.mk_rank.u32, (size_t)L * FASTF_HVG_TOP + (size_t)L * K);
    uint32_t n_lab = 0, n_per[FASTF_LABELS_MAX + 1] = {0};
    for (uint32_t c = 0; c < nc; c++) if (S->h_lab.lab[c]) { n_per[S->h_lab.lab[c] - 1]++; n_lab++; }
    for (int point = 0; point < 2; point++) {
        const res_mk_v m = res_mk_host(S, point);
        uint32_t *const rank = S->buf.mk_rank.u32 + (size_t)point * L * FASTF_HVG_TOP;
        for (uint32_t a = 0; a < L; a++) {
            m.npl[a] = n_per[a];
            for (uint32_t g = 0; g < K; g++) {
                const size_t w = (size_t)a * K + g;
                m.s2u[w] = (uint64_t)n_per[a] * (n_lab - n_per[a]) + (g + (uint32_t)point) % 2; m.sum[w] = 3 * g + a; m.det[w] = n_per[a] ? 1 : 0;
                rank[w] = point ? K - g : g + 1;
            }
        }
    }
}
static void state_free(state_t *st) { for (int i = 0; i < st->n_own; i++) free(st->own[i]); fastf_labels_free(st->labels); }

/* ---- what the public row functions give for the same arrays ---- */
typedef struct { char *p; size_t len, cap; } text_t;
static void add(text_t *t, const char *s)
{
    const size_t n = strlen(s);
    if (t->len + n + 1 > t->cap) CHECK((t->p = (char *)realloc(t->p, t->cap = (t->cap + n + 1) * 2)));
    memcpy(t->p + t->len, s, n + 1); t->len += n;
}
enum { W_SUMMARY, W_GENES, W_CELLS, W_FID, W_GFID, W_NBR, W_LAB, W_CLASSES, W_MK, W_CX, W_TABLES, P_GENES = W_TABLES, P_CELLS, P_FID, P_GFID, P_NBR, P_LAB, P_CONF, P_MK, P_CX, W_N };
static const char *const point_file[W_N] = { [P_GENES] = "genes.tsv.gz", [P_CELLS] = "cells.tsv.gz", [P_FID] = "fidelity.tsv.gz", [P_GFID] = "gene_fidelity.tsv.gz",
                                             [P_NBR] = "neighbors.tsv.gz", [P_LAB] = "labels.tsv.gz", [P_CONF] = "label_confusion.tsv.gz", [P_MK] = "markers.tsv.gz", [P_CX] = "coexpr.tsv.gz" };
static const int table_of[W_TABLES] = { -1, TB_GENES, TB_CELLS, TB_FIDELITY, TB_GENE_FIDELITY, TB_NEIGHBORS, TB_LABELS, TB_LABEL_CLASSES, TB_MARKERS, TB_COEXPR };

/* the rows of one point into want[W_*] (the tables), the texts of its files into want[P_*] (started afresh) */
static void want_point(const state_t *st, uint32_t markers, float rd, uint64_t lv, text_t *want)
{
    const res_rate_t *S = &st->S;
    const uint32_t nc = S->n_cells, nf = S->n_features, L = S->n_labels, K = S->hvg_k, top = markers < K ? markers : K;
    char row[1024], wide[64 + 4 * FASTF_LABEL_BYTES + 64], big[8 * (FASTF_LABEL_BYTES + 160)];
    const char *names[8];
    for (uint32_t l = 0; l <= L; l++) names[l] = fastf_labels_name(st->labels, l);
    for (int k = W_TABLES; k < W_N; k++) want[k].len = 0;
    CHECK(!fastf_genes_summary_row(S->rate_cell, rd, lv, S->seed, S->buf.h_cpg.u32, S->buf.h_upg.u64, nf, row, sizeof row)); add(&want[W_GENES], row);
    add(&want[P_GENES], "");
    for (uint32_t g = 0; g < nf; g++) { snprintf(row, sizeof row, "%s\t%u\t%llu\n", st->L.feat_id[g], S->buf.h_cpg.u32[g], (unsigned long long)S->buf.h_upg.u64[g]); add(&want[P_GENES], row); }
    CHECK(!fastf_cells_summary_row(S->rate_cell, rd, lv, S->seed, S->h_cs.rpc, S->h_cs.npc, S->h_cs.spc, nc, S->h_cs.hist, row, sizeof row)); add(&want[W_CELLS], row);
    add(&want[P_CELLS], "barcode\treads\tnull_umi_reads\tumis\tgenes\tsingleton_umis\tsaturation\n");
    for (uint32_t c = 0; c < nc; c++) {
        const uint64_t reads = S->h_cs.rpc[c], umis = S->buf.h_upc.u64[c];
        snprintf(row, sizeof row, "%s\t%llu\t%u\t%llu\t%u\t%u\t%.6f\n", st->L.barcode[c], (unsigned long long)reads, S->h_cs.npc[c], (unsigned long long)umis, S->buf.h_gpc.u32[c], S->h_cs.spc[c],
                 reads ? 1.0 - (double)umis / (double)reads : 0.0);
        add(&want[P_CELLS], row);
    }
    CHECK(!fastf_fidelity_summary_row(S->rate_cell, rd, lv, S->seed, S->h_fid.ufull, S->buf.h_upc.u64, S->h_fid.gfull, S->buf.h_gpc.u32, S->h_fid.sxx, S->h_fid.syy, S->h_fid.sxy, nc, nf, row, sizeof row));
    add(&want[W_FID], row); add(&want[P_FID], fastf_fidelity_header());
    for (uint32_t c = 0; c < nc; c++) {
        CHECK(!fastf_fidelity_row(st->L.barcode[c], S->h_fid.ufull[c], S->buf.h_upc.u64[c], S->h_fid.gfull[c], S->buf.h_gpc.u32[c], S->h_fid.sxx[c], S->h_fid.syy[c], S->h_fid.sxy[c], nf, row, sizeof row));
        add(&want[P_FID], row);
    }
    CHECK(!fastf_gene_fidelity_summary_row(S->rate_cell, rd, lv, S->seed, nc, S->h_gfid.sx, S->h_gfid.sy, S->h_gfid.sxx, S->h_gfid.syy, S->h_gfid.sxy, nf, row, sizeof row));
    add(&want[W_GFID], row); add(&want[P_GFID], fastf_gene_fidelity_header());
    for (uint32_t g = 0; g < nf; g++) {
        CHECK(!fastf_gene_fidelity_row(st->L.feat_id[g], nc, S->h_gfid.sx[g], S->h_gfid.sy[g], S->h_gfid.cf[g], S->h_gfid.c[g], S->h_gfid.sxx[g], S->h_gfid.syy[g], S->h_gfid.sxy[g], row, sizeof row));
        add(&want[P_GFID], row);
    }
    CHECK(!fastf_neighbors_summary_row(S->rate_cell, rd, lv, S->seed, nc, K, FASTF_NEIGHBORS_K, S->h_nbr.kf, S->h_nbr.kp, S->h_nbr.sh, row, sizeof row));
    add(&want[W_NBR], row); add(&want[P_NBR], fastf_neighbors_header());
    for (uint32_t c = 0; c < nc; c++) { CHECK(!fastf_neighbors_row(st->L.barcode[c], S->h_nbr.kf[c], S->h_nbr.kp[c], S->h_nbr.sh[c], row, sizeof row)); add(&want[P_NBR], row); }
    CHECK(!fastf_coexpr_summary_row(S->rate_cell, rd, lv, S->seed, nc, K, FASTF_COEXPR_K, S->h_cx.kf, S->h_cx.kp, S->h_cx.sh, row, sizeof row));
    add(&want[W_CX], row); add(&want[P_CX], fastf_coexpr_header());
    for (uint32_t g = 0; g < K; g++) { CHECK(!fastf_coexpr_row(st->L.feat_id[S->h_cx.genes[g]], S->h_cx.kf[g], S->h_cx.kp[g], S->h_cx.sh[g], row, sizeof row)); add(&want[P_CX], row); }
    /* labels: the row, the classes, the cells, the confusion of the point */
    const uint8_t *const lab = S->h_lab.lab;
    const uint32_t *const cx = S->h_lab.half[0].conf, *const cy = S->h_lab.half[1].conf;
    uint32_t cells[8] = {0};
    CHECK(!fastf_labels_summary_row(S->rate_cell, rd, lv, S->seed, nc, FASTF_NEIGHBORS_K, L, lab, S->h_lab.half[0].pred, S->h_lab.half[1].pred, S->h_lab.half[0].same, S->h_lab.half[0].labelled,
                                    S->h_lab.half[1].same, S->h_lab.half[1].labelled, cx, cy, row, sizeof row));
    add(&want[W_LAB], row); add(&want[P_LAB], fastf_labels_header());
    for (uint32_t c = 0; c < nc; c++) {
        cells[lab[c]]++;
        CHECK(!fastf_labels_row(st->L.barcode[c], names[lab[c]], names[S->h_lab.half[0].pred[c]], names[S->h_lab.half[1].pred[c]], S->h_lab.half[0].same[c], S->h_lab.half[0].labelled[c],
                                S->h_lab.half[1].same[c], S->h_lab.half[1].labelled[c], row, sizeof row));
        add(&want[P_LAB], row);
    }
    CHECK(!fastf_label_confusion_header(names, L, wide, sizeof wide)); add(&want[P_CONF], wide);
    for (uint32_t a = 1; a <= L; a++) {
        CHECK(!fastf_label_confusion_row(names[a], cells[a], cy + (size_t)(a - 1) * (L + 1), L, wide, sizeof wide)); add(&want[P_CONF], wide);
        CHECK(!fastf_label_classes_row(S->rate_cell, rd, lv, S->seed, names[a], a, nc, L, lab, cx, cy, row, sizeof row)); add(&want[W_CLASSES], row);
    }
    /* markers: per label the genes by ascending full rank, those in the top of either row set */
    const res_mk_v mf = res_mk_host(S, 0), mp = res_mk_host(S, 1);
    const uint32_t *const rf = res_mk_rank(S, 0), *const rp = res_mk_rank(S, 1);
    uint64_t n_lab = 0;
    CHECK(!fastf_markers_summary_rows(S->rate_cell, rd, lv, S->seed, names, L, K, markers, mf.npl, rf, rp, mf.s2u, mp.s2u, big, sizeof big)); add(&want[W_MK], big);
    add(&want[P_MK], fastf_markers_header());
    for (uint32_t a = 0; a < L; a++) n_lab += mf.npl[a];
    for (uint32_t a = 0; a < L; a++) {
        const uint32_t n_in = mf.npl[a], n_out = (uint32_t)n_lab - n_in;
        if (!n_in || !n_out) { CHECK(!fastf_markers_row(names[a + 1], NULL, n_in, n_out, 0, 0, 0, 0, 0, 0, 0, 0, 0, row, sizeof row)); add(&want[P_MK], row); continue; }
        for (uint32_t r = 1; r <= K; r++) for (uint32_t g = 0; g < K; g++) {
            const size_t w = (size_t)a * K + g;
            uint32_t det_f = 0, det_p = 0;
            if (rf[w] != r || (r > top && rp[w] > top)) continue;
            for (uint32_t o = 0; o < L; o++) { det_f += mf.det[(size_t)o * K + g]; det_p += mp.det[(size_t)o * K + g]; }
            CHECK(!fastf_markers_row(names[a + 1], st->L.feat_id[S->h_nbr.genes[g]], n_in, n_out, rf[w], rp[w], mf.s2u[w], mp.s2u[w], mf.det[w], det_f - mf.det[w], mp.det[w], det_p - mp.det[w],
                                     mp.sum[w], row, sizeof row));
            add(&want[P_MK], row);
        }
    }
}

/* ---- the runs ---- */
typedef struct { res_tsv_t tsv; res_genes_t G; res_cells_t C; res_cmp_t Fd; } tables_t;
#define ALL_FLAGS (FASTF_SWEEP_FIDELITY | FASTF_SWEEP_GENE_FIDELITY | FASTF_SWEEP_NEIGHBORS | FASTF_SWEEP_COEXPRESSION)
static void tables_open(tables_t *tb, const res_verb_t *V, const char *out, const state_t *st, uint32_t markers)
{
    memset(tb, 0, sizeof *tb);
    CHECK(!fastf_res_genes_open(&tb->G, 1, V, out, 2, 0) && !fastf_res_cells_open(&tb->C, 1, V, out) && !fastf_res_cmp_open(&tb->Fd, V, out, ALL_FLAGS, st->labels, markers, 0, NULL));
}
static void tables_point(tables_t *tb, const state_t *st, const char *name, const char *dir, float rd, uint64_t lv, res_times_t *T)
{
    const res_rate_t *S = &st->S;
    char grow[256], crow[1024];
    CHECK(!fastf_res_cmp_point(&tb->Fd, S, dir, rd, lv, T));
    CHECK(!fastf_genes_summary_row(S->rate_cell, rd, lv, S->seed, S->buf.h_cpg.u32, S->buf.h_upg.u64, S->n_features, grow, sizeof grow));
    CHECK(!fastf_res_genes_point(&tb->G, S->L, name, dir, grow, S->buf.h_cpg.u32, S->buf.h_upg.u64));
    CHECK(!fastf_cells_summary_row(S->rate_cell, rd, lv, S->seed, S->h_cs.rpc, S->h_cs.npc, S->h_cs.spc, S->n_cells, S->h_cs.hist, crow, sizeof crow));
    CHECK(!fastf_res_cells_point(&tb->C, S, dir, crow));
}
static const char *table_name(const res_verb_t *V, int table, const char *suffix)
{
    static char name[8][96]; static int at;
    at = (at + 1) % 8;
    snprintf(name[at], sizeof name[at], "%s_%s.tsv%s", V->name, fastf_res_table_stem(table), suffix);
    return name[at];
}

static int run_case(const char *tmp, int verb, uint32_t nc, uint32_t nf, uint32_t n_labels, uint32_t markers)
{
    const res_verb_t V = { .name = verb_name[verb], .index = verb, .header = summary_header[verb] };
    const float rd[2] = { verb ? 0.0f : 0.5f, verb ? 0.0f : 0.25f };
    const uint64_t lv[2] = { verb ? 100 : 0, verb ? 7 : 0 };
    static const char *const point[2] = { "p0", "p1" };
    char out[4200], dir[4300], left[2][1024], all_partial[1024];
    state_t st;
    tables_t tb;
    res_times_t T; memset(&T, 0, sizeof T);
    text_t want[W_N]; memset(want, 0, sizeof want);
    snprintf(g_case, sizeof g_case, "%s, %u cells, %u features, %u labels, --markers %u", V.name, nc, nf, n_labels, markers);
    snprintf(out, sizeof out, "%s/out", tmp);
    state_make(&st, tmp, nc, nf, n_labels);
    for (int k = 1; k < W_TABLES; k++) add(&want[k], fastf_res_table_header(verb, table_of[k]));
    {   /* what an open of everything makes, and what a run of everything leaves: with its points [0], summary only [1] */
        name_t names[W_TABLES + 3];
        for (int k = 1; k < W_TABLES; k++) strcpy(names[k - 1], table_name(&V, table_of[k], ".partial"));
        joined(names, W_TABLES - 1, all_partial);
        for (int k = 1; k < W_TABLES; k++) strcpy(names[k - 1], table_name(&V, table_of[k], ""));
        snprintf(names[W_TABLES - 1], sizeof *names, "%s_gene_cells.tsv.gz", V.name);
        joined(names, W_TABLES, left[1]);
        strcpy(names[W_TABLES], point[0]); strcpy(names[W_TABLES + 1], point[1]);
        joined(names, W_TABLES + 2, left[0]);
    }

    /* point files written; then summary only */
    for (int summary_only = 0; summary_only < 2; summary_only++) {
        CHECK(!mkdir(out, 0777));
        tables_open(&tb, &V, out, &st, markers);
        CHECK(!strcmp(listing(out), all_partial));
        for (int k = 1; k < W_TABLES; k++) want[k].len = strlen(fastf_res_table_header(verb, table_of[k]));
        for (int p = 0; p < 2; p++) {
            snprintf(dir, sizeof dir, "%s/%s", out, point[p]);
            tables_point(&tb, &st, point[p], summary_only ? NULL : dir, rd[p], lv[p], &T);
            want_point(&st, markers, rd[p], lv[p], want);
            if (summary_only) continue;
            for (int k = W_TABLES; k < W_N; k++) expect_file(dir, point_file[k], want[k].p, 1);
            CHECK(!strcmp(listing(dir), "cells.tsv.gz coexpr.tsv.gz fidelity.tsv.gz gene_fidelity.tsv.gz genes.tsv.gz label_confusion.tsv.gz labels.tsv.gz markers.tsv.gz neighbors.tsv.gz"));
        }
        CHECK(!fastf_res_genes_close(&tb.G, 1) && !fastf_res_cells_close(&tb.C, 1) && !fastf_res_cmp_close(&tb.Fd, 1));
        for (int k = 1; k < W_TABLES; k++) expect_file(out, table_name(&V, table_of[k], ""), want[k].p, 0);
        CHECK(!strcmp(listing(out), left[summary_only]));
        CHECK(T.neighbors > 0 && T.labels > 0 && T.markers > 0 && T.coexpr > 0 && T.gene_fid > 0 && T.fidelity > 0);
        remove_tree(out);
    }

    /* a failed run: nothing is left */
    CHECK(!mkdir(out, 0777));
    tables_open(&tb, &V, out, &st, markers);
    tables_point(&tb, &st, point[0], NULL, rd[0], lv[0], &T);
    CHECK(!fastf_res_genes_close(&tb.G, 0) && !fastf_res_cells_close(&tb.C, 0) && !fastf_res_cmp_close(&tb.Fd, 0));
    CHECK(!strcmp(listing(out), ""));

    /* a failed rename: the third, of <verb>_neighbors.tsv */
    {   char block[4400], inside[4500];
        memset(&tb, 0, sizeof tb);
        CHECK(!fastf_res_cmp_open(&tb.Fd, &V, out, ALL_FLAGS, st.labels, markers, 0, NULL));
        CHECK(!fastf_res_cmp_point(&tb.Fd, &st.S, NULL, rd[0], lv[0], &T));
        snprintf(block, sizeof block, "%s/%s", out, table_name(&V, TB_NEIGHBORS, ""));
        snprintf(inside, sizeof inside, "%s/keep", block);
        CHECK(!mkdir(block, 0777));
        FILE *f = fopen(inside, "w"); CHECK(f); fclose(f);
        CHECK(fastf_res_cmp_close(&tb.Fd, 1) == 1);
        CHECK(strstr(fastf_last_error(), table_name(&V, TB_NEIGHBORS, "")) && !strstr(fastf_last_error(), ".partial"));
        CHECK(!strcmp(listing(out), table_name(&V, TB_NEIGHBORS, "")) && !strcmp(listing(block), "keep"));
        CHECK(!fastf_res_cmp_close(&tb.Fd, 1));                 /* (closed: a second close does nothing) */
        remove_tree(block);
    }

    /* subsets: each comparison alone, labels without markers */
    static const struct { uint32_t flags; int labels; uint32_t markers; int table[3]; } sub[] = {
        { FASTF_SWEEP_FIDELITY, 0, 0, { TB_FIDELITY, -1, -1 } }, { FASTF_SWEEP_GENE_FIDELITY, 0, 0, { TB_GENE_FIDELITY, -1, -1 } }, { FASTF_SWEEP_NEIGHBORS, 0, 0, { TB_NEIGHBORS, -1, -1 } },
        { FASTF_SWEEP_COEXPRESSION, 0, 0, { TB_COEXPR, -1, -1 } },
        { 0, 1, 0, { TB_LABEL_CLASSES, TB_LABELS, -1 } }, { 0, 1, 1, { TB_LABEL_CLASSES, TB_LABELS, TB_MARKERS } }, { 0, 0, 0, { -1, -1, -1 } } };
    for (size_t s = 0; s < sizeof sub / sizeof *sub; s++) {
        char names[256] = "";
        for (int k = 0; k < 3; k++) if (sub[s].table[k] >= 0) { strcat(names, names[0] ? " " : ""); strcat(names, table_name(&V, sub[s].table[k], ".partial")); }
        CHECK(!fastf_res_cmp_open(&tb.Fd, &V, out, sub[s].flags, sub[s].labels ? st.labels : NULL, sub[s].markers ? markers : 0, 0, NULL));
        CHECK(!strcmp(listing(out), names));
        CHECK(!fastf_res_cmp_point(&tb.Fd, &st.S, NULL, rd[1], lv[1], &T));
        CHECK(!fastf_res_cmp_close(&tb.Fd, 0) && !strcmp(listing(out), ""));
    }
    CHECK(!rmdir(out));
    for (int k = 0; k < W_N; k++) free(want[k].p);
    state_free(&st);
    return 1;
}

int main(int argc, char **argv)
{
    static const uint32_t cells[] = { 0, 1, 5 }, features[] = { 0, 1, 4 }, labels[] = { 1, 3 }, markers[] = { 1, 3 };
    int runs = 0;
    if (argc < 2) return 9;
    for (int c = 0; c < 3; c++) for (int f = 0; f < 3; f++) for (int l = 0; l < 2; l++) for (int m = 0; m < 2; m++, runs++)
        run_case(argv[1], runs % 3, cells[c], features[f], labels[l], markers[m]);
    /* an open that fails half way takes back what it had opened: the third table's .partial is a directory */
    {   const res_verb_t V = { .name = "sweep", .index = VERB_SWEEP, .header = fastf_sweep_header };
        char out[4200], block[4400];
        res_cmp_t Fd;
        snprintf(g_case, sizeof g_case, "an open that fails");
        snprintf(out, sizeof out, "%s/out", argv[1]); snprintf(block, sizeof block, "%s/sweep_neighbors.tsv.partial", out);
        CHECK(!mkdir(out, 0777) && !mkdir(block, 0777));
        CHECK(fastf_res_cmp_open(&Fd, &V, out, ALL_FLAGS, NULL, 0, 0, NULL) == 1 && strstr(fastf_last_error(), "sweep_neighbors.tsv.partial"));
        CHECK(!strcmp(listing(out), "sweep_neighbors.tsv.partial") && !Fd.on);
        CHECK(!rmdir(block) && !rmdir(out));
    }
    printf("tables hold: %d runs\n", runs);
    return 0;
}
