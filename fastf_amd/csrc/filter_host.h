/*
 * filter_host.h — the host pieces of filter_cmds.c that fqcap_cmds.c drives too: glibc's rand() with jump-ahead, the whitelist
 * (DNA-form keys and escape prefixes), the gzip sinks and the window loop of one file.  Nothing here is exported.
 */
#ifndef FASTF_FILTER_HOST_H
#define FASTF_FILTER_HOST_H

#include "host_io.h"
#include "filter_kernels.hpp"

#include <stdio.h>
#include <time.h>
#include <zlib.h>

#define FL_HID __attribute__((visibility("hidden")))

static inline double fl_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec * 1e-9; }

/* the generator's state at output q: S[k] = r_{q+344+k}, k < 31 */
typedef struct { uint32_t r0[FLT_RAND_DEG], S[FLT_RAND_DEG]; uint64_t q; } rand_gen;
void fl_gen_seek(rand_gen *g, uint32_t seed, uint64_t q) FL_HID;
/* start states of the ceil(n / FLT_CHUNK) chunks of outputs q .. q + n - 1 into cs; the generator moves on to q + n */
void fl_gen_chunks(rand_gen *g, uint64_t n, uint32_t *cs) FL_HID;

/* whitelist: the first len bytes of every line (strncmp semantics) */
typedef struct { const char *p; uint32_t n; } fl_str;
typedef struct {
    uint64_t *dna; size_t n_dna;         /* DNA-form keys (exactly len <= 31 bases of ACGT), sorted, unique */
    fl_str *esc; size_t n_esc;           /* every other prefix, sorted */
    char *pool;
    size_t nrow;
} fl_wl;
int  fl_str_cmp(const void *a, const void *b) FL_HID;
/* get_row + read_txt of a whitelist file; keys = 0: the row count and the line-length check only.  2: the file cannot be opened */
int  fl_wl_load(fl_wl *w, const char *path, uint32_t len, int keys) FL_HID;
void fl_wl_free(fl_wl *w) FL_HID;

/* output: gzip members appended in order, or the caller's gzFile */
typedef struct { FILE *f; gzFile gz; const char *path; uint64_t bytes_in; int members; } fl_sink;
int fl_sink_open(fl_sink *s, const char *dir, const char *name, char *path, size_t path_cap) FL_HID;
int fl_sink_write(fl_sink *s, const unsigned char *p, size_t len, double *t_deflate) FL_HID;
int fl_sink_close(fl_sink *s) FL_HID;

/* what a command other than filter does with an R1 window (fl_run.hk; NULL: filter's own decision) */
typedef struct {
    int count_only;                      /* a pass that draws nothing and writes nothing: decide() also moves the '\n' carry on */
    /* the decisions of the parsed window of n_rec reads (cs: its chunk start states unless count_only); the escapes as
     * fastf_fltdev_decide returns them */
    int (*decide)(void *ctx, fastf_fltdev_t *dev, uint32_t L, const uint32_t *cs, uint64_t n_rec, const fastf_flt_esc_t **esc,
                  uint32_t *n_esc);
    /* the host's verdict on one escape: the m key bytes at p of record i of the window.  1: kept, 0: not, < 0: failed */
    int (*escape)(void *ctx, fastf_fltdev_t *dev, const unsigned char *p, uint32_t m, uint32_t i);
    void *ctx;
} fl_hooks;

typedef struct {
    fastf_fltdev_t *dev;
    size_t W;
    unsigned char *stage;                /* pinned: FLT_HDR + W + 64 */
    uint32_t len; int all; float rate; uint32_t seed;
    const fl_wl *wl;
    const fl_hooks *hk;
    uint64_t n_reads, n_kept;
    double t_fill, t_deflate, t_host, dev_ms;
    uint64_t n_escapes;
} fl_run;

/* one file through the device.  mode 0: R1 (decides, R->n_reads / n_kept out); mode 1: I1 / R2 against the bitmap, reads >= limit
 * ignored.  `name` names the file in messages. */
int fl_file(fl_run *R, fq_src *src, int mode, uint64_t limit, const char *name, fl_sink *sink) FL_HID;

/* dir exists and the wanted names can be created or rewritten in it */
int fl_dir_writable(const char *dir, const char *const names[], const int want[], int n) FL_HID;

#endif
