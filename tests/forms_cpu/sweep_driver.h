// The sweep of tests/test_forms_cpu.py: every row count 1 .. 1408 and 2048 x vertex sets x weights per vertex x scene sizes, one line
// per RUN of rows over which a plan does not change.  A line:
//   key <TAB> first row <TAB> last row <TAB> the plan's fields that hold for the whole run <TAB> the per-row fields (grid, workgroup
//   map) at the first row <TAB> ... at the last row <TAB> FNV-1a of the per-row fields of every row of the run
// The includer defines the ev_* functions (the plans of csrc/fdc_forms.h as text) and g_nn_mode before including this file.
// argv: NAME=VALUE pairs, put into the environment before the first plan is asked for; NN_MODE=k is fdcap_set_nn_kernel(k);
// --every-row: one line per row instead of one per run; @kind:rows:nv[:c[:d]] (kind = a key's first word, then its parameters in the
// key's order): that one point instead of the sweep.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

struct Rec { std::string plan, per_row; };

static int g_nn_mode = 0;
Rec ev_pfwd(int rows, int nv);                       // blend forward as its own launch
Rec ev_cfwd(int rows, int nv, int wpv, int ja);      // contact forward: fused or two launches
Rec ev_bwd(int rows, int nv, bool may_split);        // blend data gradient
Rec ev_skin(int rows, int nv, int wpv);              // the contact set's skinning backward
Rec ev_skinany(int rows, int nv);                    // skin_bwd_kernel for any vertex set
Rec ev_nn(int rows, int nv, int ns);                 // the in-loop search (+ the splits its buffers are sized for)

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// fields that are zero are left out of a line (most of a plan's parameters belong to one form only)
static std::string drop_zero_fields(const std::string& s) {
    std::string out;
    for (size_t i = 0; i < s.size();) {
        size_t j = s.find(' ', i);
        if (j == std::string::npos) j = s.size();
        const std::string tok = s.substr(i, j - i);
        const size_t eq = tok.find('=');
        if (eq == std::string::npos || tok.find_first_not_of("0,", eq + 1) != std::string::npos) out += (out.empty() ? "" : " ") + tok;
        i = j + 1;
    }
    return out;
}

static bool g_every_row = false;

template <class F>
static void sweep_rows(const std::string& key, F ev_raw) {
    const auto ev = [&](int r) { Rec c = ev_raw(r); c.plan = drop_zero_fields(c.plan); c.per_row = drop_zero_fields(c.per_row); return c; };
    std::vector<int> rows;
    for (int r = 1; r <= 1408; ++r) rows.push_back(r);
    rows.push_back(2048);
    Rec first, last;
    int r0 = 0, r1 = 0;
    uint64_t h = 0;
    const auto flush = [&]() {
        if (r0) printf("%s\t%d\t%d\t%s\t%s\t%s\t%016llx\n", key.c_str(), r0, r1, first.plan.c_str(), first.per_row.c_str(), last.per_row.c_str(), (unsigned long long)h);
    };
    for (int r : rows) {
        const Rec c = ev(r);
        if (!r0 || c.plan != first.plan || g_every_row) { flush(); first = c; r0 = r; h = 1469598103934665603ull; }
        for (unsigned char ch : c.per_row + ";") { h ^= ch; h *= 1099511628211ull; }
        last = c; r1 = r;
    }
    flush();
}

static void point(const char* q) {
    char kind[16] = "";
    int a[4] = {0, 0, 0, 0};
    sscanf(q, "@%15[a-z]:%d:%d:%d:%d", kind, &a[0], &a[1], &a[2], &a[3]);
    const std::string k = kind;
    Rec c;
    if (k == "pfwd") c = ev_pfwd(a[0], a[1]);
    else if (k == "bwd") c = ev_bwd(a[0], a[1], a[2] != 0);
    else if (k == "skinany") c = ev_skinany(a[0], a[1]);
    else if (k == "cfwd") c = ev_cfwd(a[0], a[1], a[2], a[3]);
    else if (k == "skin") c = ev_skin(a[0], a[1], a[2]);
    else if (k == "nn") c = ev_nn(a[0], a[1], a[2]);
    else { fprintf(stderr, "unknown query %s\n", q); exit(2); }
    printf("%s\t%s\t%s\n", q, drop_zero_fields(c.plan).c_str(), drop_zero_fields(c.per_row).c_str());
}

int main(int argc, char** argv) {
    std::vector<const char*> points;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--every-row")) { g_every_row = true; continue; }
        if (argv[i][0] == '@') { points.push_back(argv[i]); continue; }
        char* eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "usage: %s [NAME=VALUE ...]\n", argv[0]); return 2; }
        const std::string name(argv[i], eq - argv[i]);
        if (name == "NN_MODE") g_nn_mode = atoi(eq + 1);
        else setenv(name.c_str(), eq + 1, 1);
    }
    for (const char* q : points) point(q);
    if (!points.empty()) return 0;
    const int sets[] = {100, 220, 500, 512, 560, 700, 840, 1000, 1024, 1025, 4000, 10475};
    const int wpvs[] = {4, 8, 12};
    const int scenes[] = {20000, 100000, 500000, 2000000};
    for (int nv : sets) {
        sweep_rows(fmt("pfwd nv=%d", nv), [&](int r) { return ev_pfwd(r, nv); });
        for (int sp = 0; sp < 2; ++sp) sweep_rows(fmt("bwd nv=%d may_split=%d", nv, sp), [&](int r) { return ev_bwd(r, nv, sp != 0); });
        sweep_rows(fmt("skinany nv=%d", nv), [&](int r) { return ev_skinany(r, nv); });
        for (int wpv : wpvs) {
            // ja: joints the set's weights reach -- 37 is the most the fused forward's LDS budget admits, 38 the least it does not
            for (int ja : {37, 38}) sweep_rows(fmt("cfwd nv=%d wpv=%d ja=%d", nv, wpv, ja), [&](int r) { return ev_cfwd(r, nv, wpv, ja); });
            sweep_rows(fmt("skin nv=%d wpv=%d", nv, wpv), [&](int r) { return ev_skin(r, nv, wpv); });
        }
        // (the search sees a set only through rows x vertices: four of the sets keep the table small)
        if (nv == 100 || nv == 500 || nv == 1024 || nv == 10475)
            for (int ns : scenes) sweep_rows(fmt("nn nv=%d ns=%d", nv, ns), [&](int r) { return ev_nn(r, nv, ns); });
    }
    return 0;
}
