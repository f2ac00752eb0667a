/* cli_opts.c — the option scanner of the commands (cli_opts.h): both dialects, and the five messages of an option error */
#include "cli_opts.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const cli_opt *cli_fail(cli_scan *s, int err, const char *fmt, const char *what)
{
    fprintf(stderr, fmt, what);
    s->err = err;
    return NULL;
}

const cli_opt *cli_next(cli_scan *s)
{
    const cli_opt *o = NULL;
    const char *p = s->rest, *glued = NULL;                  /* p: the letter looked at; glued: a value in the same argument */
    if (s->err) return NULL;
    s->val = s->rest = NULL;
    if (!p) {                                                /* the next argument */
        for (;;) {
            if (++s->i >= s->argc) return NULL;
            p = s->argv[s->i];
            if (p[0] == '-' && p[1]) break;
            if (!(s->flags & CLI_ARGPARSE)) return NULL;     /* no option, or a lone `-`: skipped or the end */
        }
        if (p[1] == '-' && !p[2]) return NULL;               /* `--` */
        p++;
    }
    const char *a = s->argv[s->i];
    if (a[1] == '-') {
        const char *eq = strchr(a + 2, '=');
        const size_t nl = eq ? (size_t)(eq - a - 2) : strlen(a + 2);
        for (const cli_opt *k = s->opts; k->l && !o; k++) if (strlen(k->l) == nl && !strncmp(k->l, a + 2, nl)) o = k;
        if (o) snprintf(s->name, sizeof s->name, "--%s", o->l);
        if (o && eq) glued = eq + 1;
    } else {
        for (const cli_opt *k = s->opts; k->l && !o; k++) if (k->s == *p) o = k;
        if (o) snprintf(s->name, sizeof s->name, "-%c", o->s);
        if (o && p[1]) { if (o->has_arg) glued = p + 1; else if (s->flags & CLI_ARGPARSE) s->rest = p + 1; }
    }
    if (!o) return cli_fail(s, CLI_UNKNOWN, "error: unknown option `%s`\n", a);
    if (o->has_arg) {
        if (!glued && s->i + 1 >= s->argc) return cli_fail(s, CLI_NO_VALUE, "error: option `%s` requires a value\n", s->name);
        s->val = glued ? glued : s->argv[++s->i];
    }
    return o;
}

/* argparse.c:88-108: ERANGE first, then trailing characters; an empty value parses as 0 */
static void cli_number_checked(cli_scan *s, int erange, const char *end, const char *expects)
{
    const char *why = erange ? "numerical result out of range" : *end ? expects : NULL;
    if (!why) return;
    fprintf(stderr, "error: option `%s` %s\n", s->name, why);
    s->err = CLI_BAD_VALUE;
}

long cli_int(cli_scan *s)
{
    char *end = NULL;
    errno = 0;
    const long v = strtol(s->val, &end, 0);
    cli_number_checked(s, errno == ERANGE && !(s->flags & CLI_NO_ERANGE), end, "expects an integer value");
    return v;
}

float cli_float(cli_scan *s)
{
    char *end = NULL;
    errno = 0;
    const float v = strtof(s->val, &end);
    cli_number_checked(s, errno == ERANGE, end, "expects a numerical value");
    return v;
}
