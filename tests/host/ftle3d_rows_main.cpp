// Stand-alone host check of smk_ftle3d_field's row map and group rule (smokephysai_amd/csrc/flow_map3d.h: the text the kernel, the
// launcher and the workspace query compile).  For every shape and pitch: one volume [D][H][pitch_m] of counters, laid out as the entry
// point takes a displacement component or the FTLE, with its pitch padding; the program walks the groups and their rows exactly as
// k3_ftle does (group p owns rows [p * rpg, min((p + 1) * rpg, D H)), a row's columns 0 .. W - 1 at offset + c) and counts every visit.
// Checked: every cell [plane][row][col < W] is visited exactly once; no padding element is visited; no offset leaves the volume; the
// groups tile the rows (no empty group, at most FM3_MAX_P of them, at least FM3_ROWS rows each but the last); (plane, row) are those of
// the offset; the workspace the query returns, fm3_workspace_bytes, is what the launch writes: one (sum, maximum) pair of doubles per grid
// and group.  Built by tests/test_ftle3d_rows_host.py with the host compiler, with the address and undefined-behaviour sanitizers where
// the toolchain has them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "flow_map3d.h"

using namespace smk;

static long long violations = 0;
static void fail(const char *what, int D, int H, int W, int pm, long long a, long long b) {
    if (violations++ < 20) printf("VIOLATION %s at %dx%dx%d pitch %d: %lld %lld\n", what, D, H, W, pm, a, b);
}

int main(int argc, char **argv) {
    if (argc < 2 || strcmp(argv[1], "walk") != 0) {
        printf("usage: ftle3d_rows walk\n");
        return 2;
    }
    const int shapes[][3] = {{3, 3, 3}, {4, 5, 7}, {6, 12, 16}, {6, 19, 37}, {9, 19, 37}, {12, 33, 40}, {16, 272, 8},
                             {64, 128, 128}, {3, 700, 5}, {700, 3, 5}, {300, 300, 3}};
    const int pads[] = {0, 5, 25};                                   // pitch_m = W + pad
    const int B = 2;
    long long cases = 0, elements = 0, rows_total = 0, groups_total = 0, workspace_total = 0, longest_run = 0;
    for (const auto &s : shapes) {
        for (const int pad : pads) {
            const int D = s[0], H = s[1], W = s[2], pm = W + pad;
            ++cases;
            if (!fm3_pitch_ok(D, H, W, pm)) fail("pitch refused", D, H, W, pm, 0, 0);
            const int64_t size = (int64_t)D * H * pm;
            std::vector<uint8_t> hits((size_t)size, (uint8_t)0);
            const int64_t rows = fm3_rows(D, H);
            const int rpg = fm3_rows_per_group(D, H), groups = fm3_groups(D, H);
            if (rows != (int64_t)D * H) fail("row count", D, H, W, pm, rows, (int64_t)D * H);
            if (rpg < FM3_ROWS) fail("rows per group below FM3_ROWS", D, H, W, pm, rpg, FM3_ROWS);
            if (groups < 1 || groups > FM3_MAX_P) fail("group count", D, H, W, pm, groups, FM3_MAX_P);
            if ((int64_t)groups * rpg < rows || (int64_t)(groups - 1) * rpg >= rows) fail("groups do not tile the rows", D, H, W, pm, groups, rpg);
            if (rpg > longest_run) longest_run = rpg;
            int64_t next = 0;                                        // the rows arrive in ascending order, each once
            for (int p = 0; p < groups; ++p) {
                const int64_t r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
                if (r0 != next || r1 <= r0) fail("group run", D, H, W, pm, r0, next);
                for (int64_t r = r0; r < r1; ++r) {
                    const Fm3Row q = fm3_row(H, pm, r);
                    if (q.plane < 0 || q.plane >= D || q.row < 0 || q.row >= H) { fail("plane or row", D, H, W, pm, q.plane, q.row); continue; }
                    if (q.offset != ((int64_t)q.plane * H + q.row) * pm) fail("offset", D, H, W, pm, r, q.offset);
                    if (q.offset < 0 || q.offset + W > size) { fail("offset leaves the volume", D, H, W, pm, r, q.offset); continue; }
                    for (int c = 0; c < W; ++c) {
                        uint8_t &h = hits[(size_t)(q.offset + c)];
                        if (h < 255) ++h;
                    }
                }
                next = r1;
            }
            if (next != rows) fail("rows left over", D, H, W, pm, next, rows);
            for (int64_t i = 0; i < size; ++i) {
                const bool live = i % pm < W;
                if (hits[(size_t)i] != (live ? 1 : 0)) fail(live ? "cell not visited exactly once" : "padding visited", D, H, W, pm, i, hits[(size_t)i]);
                elements += live;
            }
            rows_total += rows;
            groups_total += groups;
            if (fm3_workspace_bytes(B, D, H) != (int64_t)groups * B * 2 * 8) fail("workspace", D, H, W, pm, fm3_workspace_bytes(B, D, H), groups);
            workspace_total += fm3_workspace_bytes(B, D, H);         // what smk_ftle3d_workspace(B, D, H, W) returns
        }
    }
    printf("CASES %lld ELEMENTS %lld ROWS %lld GROUPS %lld WORKSPACE %lld LONGEST %lld VIOLATIONS %lld\n", cases, elements, rows_total,
           groups_total, workspace_total, longest_run, violations);
    return violations ? 1 : 0;
}
