/*
 * cli_opts.h — the one option scanner of the commands' command lines (argparse.c:36-117, 149-287 restated).
 *
 * A command hands cli_next() a table of cli_opt and switches over what comes back.  Two dialects:
 *   default        bam2db, crb, extract, sweep, cap, level: the first argument that is no option, a lone `-` and `--` end the
 *                  parsing; `-xVALUE`, `-x VALUE`, `--long VALUE`, `--long=VALUE`; a flag ignores what is glued behind its letter
 *   CLI_ARGPARSE   freq, filter: arguments that are no options are skipped, `--` ends the parsing; the short options cluster
 *                  (`-al16`), the rest of a cluster being the value of the first option that takes one
 * Long names match whole, up to the end or the `=`.  An unknown option, a missing value and a bad number are reported on stderr
 * in argparse.c's words, naming the option as it was spelled (`--seed`, `-s`); cli_next() then returns NULL with `err` set, and
 * the command prints its usage (or not) and ends as it always did.  No global state, nothing allocated.
 */
#ifndef FASTF_CLI_OPTS_H
#define FASTF_CLI_OPTS_H

typedef struct { char s; const char *l; int has_arg; } cli_opt;      /* s == 0: no short form; the table ends with l == NULL */

enum { CLI_ARGPARSE = 1, CLI_NO_ERANGE = 2 };                        /* flags; NO_ERANGE: cli_int() as `extract -T`, no range check */
enum { CLI_UNKNOWN = 1, CLI_NO_VALUE, CLI_BAD_VALUE };               /* err */

typedef struct {
    int argc; const char **argv; const cli_opt *opts; unsigned flags;   /* set by the caller; everything below starts as 0 */
    int i;                      /* the argument looked at last */
    const char *rest;           /* CLI_ARGPARSE: what is left of a cluster */
    const char *val;            /* the value of the option returned last, NULL for a flag */
    char name[40];              /* its spelling */
    int err;
} cli_scan;

#define CLI_SCAN(argc, argv, opts, flags) { (argc), (argv), (opts), (flags), 0, NULL, NULL, "", 0 }

/* the next option; NULL at the end of the options (err == 0) or after a message */
const cli_opt *cli_next(cli_scan *s) __attribute__((visibility("hidden")));
/* s->val through strtol(v, &end, 0) or strtof: ERANGE first, then trailing characters; an empty value is 0.  After a message err is
 * set and the next cli_next() returns NULL */
long cli_int(cli_scan *s) __attribute__((visibility("hidden")));
float cli_float(cli_scan *s) __attribute__((visibility("hidden")));

#endif
