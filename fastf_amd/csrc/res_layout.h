/* res_layout.h — the carved blocks of the pair state (resident.h: res_rate_t).  ONE function per block: from a base pointer and the counts
 * the block is laid out for it gives the typed arrays inside the block and the bytes of the whole.  fastf_res_rate_open sizes a block by
 * it (base NULL: the arrays are NULL, .bytes is what counts) and every consumer takes its pointers from it, so the order of the arrays
 * inside a block is written here and nowhere else.  Arrays follow each other without padding but where a count below says so.
 * Plain C, no HIP and no other header of the project: tools/res_layout_check.c includes this alone. */
#ifndef FASTF_RES_LAYOUT_H
#define FASTF_RES_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

typedef struct { char *base; size_t off; } res_carve_t;
static inline void *res_carve_(res_carve_t *c, size_t n, size_t elem) { void *const p = c->base ? c->base + c->off : NULL; c->off += n * elem; return p; }
#define RES_CARVE(c, field, n) ((field) = res_carve_(&(c), (n), sizeof *(field)))

/* the rows of a row set: feature, cell, count, N entries apart (N: the records of the run) */
typedef struct { uint32_t *f, *c, *k; } res_rows_t;
static inline res_rows_t res_rows(void *base, size_t N) { res_rows_t r; r.f = (uint32_t *)base; r.c = r.f + N; r.k = r.c + N; return r; }

/* --cells: the copy-number histogram (RES_CELLS_HIST_BYTES hold its FASTF_COPY_BINS + 1 words), then reads, UMIs-with-copies and
 * singletons per cell; the device block and its pinned copy, which one transfer fills */
#define RES_CELLS_HIST_BYTES 512u
typedef struct { uint64_t *hist; uint32_t *rpc, *npc, *spc; size_t bytes; } res_cellsum_v;
static inline res_cellsum_v res_cellsum_layout(void *base, size_t n_cells)
{
    res_carve_t c = { (char *)base, 0 }; res_cellsum_v v;
    RES_CARVE(c, v.hist, RES_CELLS_HIST_BYTES / sizeof *v.hist); RES_CARVE(c, v.rpc, n_cells); RES_CARVE(c, v.npc, n_cells); RES_CARVE(c, v.spc, n_cells);
    v.bytes = c.off; return v;
}

/* level: lo, hi, the probes and U_k(2^32) of the search, per cell */
typedef struct { uint64_t *lo, *hi, *probe, *ufull; size_t bytes; } res_level_v;
static inline res_level_v res_level_layout(void *base, size_t n)
{
    res_carve_t c = { (char *)base, 0 }; res_level_v v;
    RES_CARVE(c, v.lo, n); RES_CARVE(c, v.hi, n); RES_CARVE(c, v.probe, n); RES_CARVE(c, v.ufull, n);
    v.bytes = c.off; return v;
}

/* --fidelity: sum_xy, sum_yy, sum_xx per cell; the pinned block has umis_full (n_cells + 1 used) and genes_full of the pair behind them */
typedef struct { uint64_t *sxy, *syy, *sxx, *ufull; uint32_t *gfull; size_t bytes; } res_fid_v;
static inline res_fid_v res_fid_layout(void *base, size_t n, int pinned)
{
    res_carve_t c = { (char *)base, 0 }; res_fid_v v;
    RES_CARVE(c, v.sxy, n); RES_CARVE(c, v.syy, n); RES_CARVE(c, v.sxx, n); RES_CARVE(c, v.ufull, pinned ? n : 0); RES_CARVE(c, v.gfull, pinned ? n : 0);
    v.bytes = c.off; return v;
}

/* --gene-fidelity: per gene sum_x, sum_xx (the pair's), sum_y, sum_yy, sum_xy (a point's), then cells_full and cells; the device block
 * and its pinned copy alike */
typedef struct { uint64_t *sx, *sxx, *sy, *syy, *sxy; uint32_t *cf, *c; size_t bytes; } res_gfid_v;
static inline res_gfid_v res_gfid_layout(void *base, size_t n)
{
    res_carve_t c = { (char *)base, 0 }; res_gfid_v v;
    RES_CARVE(c, v.sx, n); RES_CARVE(c, v.sxx, n); RES_CARVE(c, v.sy, n); RES_CARVE(c, v.syy, n); RES_CARVE(c, v.sxy, n); RES_CARVE(c, v.cf, n); RES_CARVE(c, v.c, n);
    v.bytes = c.off; return v;
}

/* --neighbors.  The slot map of A: u16[n_features + 1] in map_bytes (res_nbr_map_bytes: a multiple of 8).  The device block: the map, the
 * norms, the neighbour indices (k a cell) of the full rows [0] and of the point [1], their counts, the shared counts.  The pinned block:
 * the map, k_full, k_point, shared and the genes of A in rank order (n_genes: FASTF_HVG_TOP) */
static inline size_t res_nbr_map_bytes(size_t n_features) { return ((n_features + 1) * sizeof(uint16_t) + 7) & ~(size_t)7; }
typedef struct { uint16_t *map; uint64_t *norms; uint32_t *idx[2], *cnt[2], *shared; size_t bytes; } res_nbr_v;
static inline res_nbr_v res_nbr_layout(void *base, size_t map_bytes, size_t k, size_t nc)
{
    res_carve_t c = { (char *)base, 0 }; res_nbr_v v;
    RES_CARVE(c, v.map, map_bytes / sizeof *v.map); RES_CARVE(c, v.norms, nc); RES_CARVE(c, v.idx[0], nc * k); RES_CARVE(c, v.idx[1], nc * k);
    RES_CARVE(c, v.cnt[0], nc); RES_CARVE(c, v.cnt[1], nc); RES_CARVE(c, v.shared, nc);
    v.bytes = c.off; return v;
}
typedef struct { uint16_t *map; uint32_t *kf, *kp, *sh, *genes; size_t bytes; } res_nbr_pin_v;
static inline res_nbr_pin_v res_nbr_pin_layout(void *base, size_t map_bytes, size_t nc, size_t n_genes)
{
    res_carve_t c = { (char *)base, 0 }; res_nbr_pin_v v;
    RES_CARVE(c, v.map, map_bytes / sizeof *v.map); RES_CARVE(c, v.kf, nc); RES_CARVE(c, v.kp, nc); RES_CARVE(c, v.sh, nc); RES_CARVE(c, v.genes, n_genes);
    v.bytes = c.off; return v;
}

/* --mapping.  The device block: the norms of the full rows (the norms of res_nbr_v are the row set's at hand: every point overwrites
 * them) M(i) (k a cell) and the confusion counts the vote call fills beside its
 * votes (n_labels x (n_labels + 1), not used further), then — 8-byte aligned — the part that leaves in ONE copy of out_bytes from `sd` on, into the pinned block,
 * which is that part alone: self_dot, self_rank, k_map (the counts of M), hood, and pred, same, labelled (u8, lab_cells each:
 * res_lab_cells; 0 without --labels) */
typedef struct { uint64_t *norms; uint32_t *idx, *conf; uint64_t *sd; uint32_t *rank, *km, *hood; uint8_t *pred, *same, *labelled; size_t out_bytes, bytes; } res_map_v;
static inline res_map_v res_map_layout(void *base, size_t k, size_t nc, size_t lab_cells, size_t n_labels, int pinned)
{
    res_carve_t c = { (char *)base, 0 }; res_map_v v;
    RES_CARVE(c, v.norms, pinned ? 0 : nc); RES_CARVE(c, v.idx, pinned ? 0 : nc * k); RES_CARVE(c, v.conf, pinned ? 0 : n_labels * (n_labels + 1));
    const size_t out = c.off = (c.off + 7) & ~(size_t)7;
    RES_CARVE(c, v.sd, nc); RES_CARVE(c, v.rank, nc); RES_CARVE(c, v.km, nc); RES_CARVE(c, v.hood, nc);
    RES_CARVE(c, v.pred, lab_cells); RES_CARVE(c, v.same, lab_cells); RES_CARVE(c, v.labelled, lab_cells);
    v.out_bytes = c.off - out; v.bytes = c.off; return v;
}

/* --coexpression, over the K genes of A (FASTF_HVG_TOP at the most).  The device block: D (K x K) and S of the row set at hand, the slot
 * map of A (map_bytes, as above: the option keeps its own, so that it runs without --neighbors), the partner slots (k a gene) of the full
 * rows [0] and of the point [1], their counts, the shared counts.  The pinned block: the map, k_full, k_point, shared and the genes of A
 * in rank order */
typedef struct { uint64_t *D, *S; uint16_t *map; uint32_t *idx[2], *cnt[2], *shared; size_t bytes; } res_cx_v;
static inline res_cx_v res_cx_layout(void *base, size_t map_bytes, size_t k, size_t K)
{
    res_carve_t c = { (char *)base, 0 }; res_cx_v v;
    RES_CARVE(c, v.D, K * K); RES_CARVE(c, v.S, K); RES_CARVE(c, v.map, map_bytes / sizeof *v.map); RES_CARVE(c, v.idx[0], K * k); RES_CARVE(c, v.idx[1], K * k);
    RES_CARVE(c, v.cnt[0], K); RES_CARVE(c, v.cnt[1], K); RES_CARVE(c, v.shared, K);
    v.bytes = c.off; return v;
}
typedef struct { uint16_t *map; uint32_t *kf, *kp, *sh, *genes; size_t bytes; } res_cx_pin_v;
static inline res_cx_pin_v res_cx_pin_layout(void *base, size_t map_bytes, size_t K)
{
    res_carve_t c = { (char *)base, 0 }; res_cx_pin_v v;
    RES_CARVE(c, v.map, map_bytes / sizeof *v.map); RES_CARVE(c, v.kf, K); RES_CARVE(c, v.kp, K); RES_CARVE(c, v.sh, K); RES_CARVE(c, v.genes, K);
    v.bytes = c.off; return v;
}

/* --labels: lab of the pair's cells, then one half for the full rows [0] and one for the point [1] — pred, same, labelled (u8) and conf
 * (u32, n_labels x (n_labels + 1)); a half starts at its pred and leaves in one copy of half_bytes.  lab_cells: res_lab_cells(cells), a
 * multiple of 4, which keeps conf aligned.  The device block and its pinned copy alike */
static inline size_t res_lab_cells(size_t cells) { return (cells + 3) & ~(size_t)3; }
typedef struct { uint8_t *lab; struct { uint8_t *pred, *same, *labelled; uint32_t *conf; } half[2]; size_t half_bytes, bytes; } res_lab_v;
static inline res_lab_v res_lab_layout(void *base, size_t lab_cells, size_t n_labels)
{
    res_carve_t c = { (char *)base, 0 }; res_lab_v v;
    RES_CARVE(c, v.lab, lab_cells);
    for (int h = 0; h < 2; h++) {
        RES_CARVE(c, v.half[h].pred, lab_cells); RES_CARVE(c, v.half[h].same, lab_cells); RES_CARVE(c, v.half[h].labelled, lab_cells);
        RES_CARVE(c, v.half[h].conf, n_labels * (n_labels + 1));
    }
    v.half_bytes = (c.off - lab_cells) / 2; v.bytes = c.off; return v;
}

/* --pseudotime: t of the pair's cells, then one half for the full rows [0], one for the point [1] and one for the mapping list [2] — the
 * census (8 u64: FASTF_PTIME_OUT_WORDS used), est and valued (u32 per cell); a half starts at its census and leaves in one copy of
 * half_bytes.  pt_cells: res_pt_cells(cells), an even number, which keeps every census aligned.  The device block and its pinned copy alike */
#define RES_PT_CENSUS_WORDS 8u
static inline size_t res_pt_cells(size_t cells) { return (cells + 1) & ~(size_t)1; }
typedef struct { uint32_t *t; struct { uint64_t *census; uint32_t *est, *valued; } half[3]; size_t half_bytes, bytes; } res_pt_v;
static inline res_pt_v res_pt_layout(void *base, size_t pt_cells)
{
    res_carve_t c = { (char *)base, 0 }; res_pt_v v;
    RES_CARVE(c, v.t, pt_cells);
    for (int h = 0; h < 3; h++) { RES_CARVE(c, v.half[h].census, RES_PT_CENSUS_WORDS); RES_CARVE(c, v.half[h].est, pt_cells); RES_CARVE(c, v.half[h].valued, pt_cells); }
    v.half_bytes = (c.off - pt_cells * sizeof *v.t) / 3; v.bytes = c.off; return v;
}

/* --markers: the four tables of ONE row set — s2u, sum (u64), det (u32), n_labels x K each, then n_per_label (u32, an even number of
 * entries) — which leave the device in one copy of .bytes.  The pinned block holds two sets, res_mk_set_bytes apart */
typedef struct { uint64_t *s2u, *sum; uint32_t *det, *npl; size_t bytes; } res_mk_v;
static inline res_mk_v res_mk_layout(void *base, size_t n_labels, size_t K)
{
    res_carve_t c = { (char *)base, 0 }; res_mk_v v;
    RES_CARVE(c, v.s2u, n_labels * K); RES_CARVE(c, v.sum, n_labels * K); RES_CARVE(c, v.det, n_labels * K); RES_CARVE(c, v.npl, (n_labels + 1) & ~(size_t)1);
    v.bytes = c.off; return v;
}
static inline size_t res_mk_set_bytes(size_t n_labels, size_t K) { return (res_mk_layout(NULL, n_labels, K).bytes + 7) & ~(size_t)7; }

#endif
