// Stand-alone host check of smk_tangent3d_renorm's row map and group rule (smokephysai_amd/csrc/fluid_tangent3d.h: the text the kernels, the
// launcher and the workspace query compile).  For every shape and pitch pair: the five fields of a tangent state are laid out as the
// entry point takes them, each with its pitch padding, in one array of counters; the program walks the groups and their rows exactly as
// k3_tangent_sumsq / k3_tangent_scale do (group p owns rows [p * rpg, min((p + 1) * rpg, rows)), a row's columns 0 .. cols - 1 at
// offset + c of its field) and counts every visit.  Checked: every element [plane][row][col < columns] of the five fields is visited
// exactly once; no padding element is visited; no offset leaves its field; the groups tile the rows (no empty group, at most FT3_MAX_P
// of them, at least FT3_ROWS rows each but the last); (field, plane, row) are those of the offset; the workspace the query would return,
// groups * B * T * 8, is what the launch writes.  Built by tests/test_tangent3d_rows_host.py with the host compiler, with the address and
// undefined-behaviour sanitizers where the toolchain has them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fluid_tangent3d.h"

using namespace smk;

static long long violations = 0;
static void fail(const char *what, int D, int H, int W, int pc, int pv, long long a, long long b) {
    if (violations++ < 20) printf("VIOLATION %s at %dx%dx%d pitches %d %d: %lld %lld\n", what, D, H, W, pc, pv, a, b);
}

int main(int argc, char **argv) {
    if (argc < 2 || strcmp(argv[1], "walk") != 0) {
        printf("usage: tangent3d_rows walk\n");
        return 2;
    }
    const int shapes[][3] = {{3, 3, 3}, {4, 5, 7}, {6, 19, 37}, {9, 19, 37}, {12, 33, 40}, {64, 128, 128}, {3, 700, 5}, {700, 3, 5}};
    const int pads[][2] = {{0, 0}, {3, 2}, {25, 1}};                 // pitch_c = W + pads[0], pitch_v = W + 1 + pads[1]
    const int B = 2, T = 2;
    long long cases = 0, elements = 0, rows_total = 0, groups_total = 0, workspace_total = 0;
    for (const auto &s : shapes) {
        for (const auto &pad : pads) {
            const int D = s[0], H = s[1], W = s[2], pc = W + pad[0], pv = W + 1 + pad[1];
            ++cases;
            const int64_t size[5] = {(int64_t)D * (H + 1) * pc, (int64_t)D * H * pv, (int64_t)(D + 1) * H * pc, (int64_t)D * H * pc,
                                     (int64_t)D * H * pc};
            const int planes[5] = {D, D, D + 1, D, D}, rpp[5] = {H + 1, H, H, H, H}, cols[5] = {W, W + 1, W, W, W},
                      pitch[5] = {pc, pv, pc, pc, pc};
            std::vector<std::vector<uint8_t>> hits;
            for (int f = 0; f < 5; ++f) hits.emplace_back((size_t)size[f], (uint8_t)0);
            const int64_t rows = ft3_rows(D, H);
            const int rpg = ft3_rows_per_group(D, H), groups = ft3_groups(D, H);
            int64_t want_rows = 0;
            for (int f = 0; f < 5; ++f) want_rows += (int64_t)planes[f] * rpp[f];
            if (rows != want_rows) fail("row count", D, H, W, pc, pv, rows, want_rows);
            if (rpg < FT3_ROWS) fail("rows per group below FT3_ROWS", D, H, W, pc, pv, rpg, FT3_ROWS);
            if (groups < 1 || groups > FT3_MAX_P) fail("group count", D, H, W, pc, pv, groups, FT3_MAX_P);
            if ((int64_t)groups * rpg < rows || (int64_t)(groups - 1) * rpg >= rows) fail("groups do not tile the rows", D, H, W, pc, pv, groups, rpg);
            int64_t next = 0;                                        // the rows arrive in ascending order, each once
            for (int p = 0; p < groups; ++p) {
                const int64_t r0 = (int64_t)p * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
                if (r0 != next || r1 <= r0) fail("group run", D, H, W, pc, pv, r0, next);
                for (int64_t r = r0; r < r1; ++r) {
                    const Ft3Row q = ft3_row(D, H, W, pc, pv, r);
                    if (q.field < 0 || q.field > 4) { fail("field", D, H, W, pc, pv, r, q.field); continue; }
                    const int f = q.field;
                    if (q.cols != cols[f]) fail("columns", D, H, W, pc, pv, r, q.cols);
                    if (q.plane < 0 || q.plane >= planes[f] || q.row < 0 || q.row >= rpp[f]) fail("plane or row", D, H, W, pc, pv, q.plane, q.row);
                    if (q.offset != ((int64_t)q.plane * rpp[f] + q.row) * pitch[f]) fail("offset", D, H, W, pc, pv, r, q.offset);
                    if (q.offset < 0 || q.offset + q.cols > size[f]) { fail("offset leaves the field", D, H, W, pc, pv, r, q.offset); continue; }
                    for (int c = 0; c < q.cols; ++c) {
                        uint8_t &h = hits[f][(size_t)(q.offset + c)];
                        if (h < 255) ++h;
                    }
                }
                next = r1;
            }
            if (next != rows) fail("rows left over", D, H, W, pc, pv, next, rows);
            for (int f = 0; f < 5; ++f) {
                for (int64_t i = 0; i < size[f]; ++i) {
                    const bool live = i % pitch[f] < cols[f];
                    if (hits[f][(size_t)i] != (live ? 1 : 0)) fail(live ? "element not visited exactly once" : "padding visited", D, H, W, pc, pv, f, i);
                    elements += live;
                }
            }
            rows_total += rows;
            groups_total += groups;
            workspace_total += (int64_t)groups * B * T * 8;          // what smk_tangent3d_renorm_workspace(B, T, D, H, W) returns
        }
    }
    printf("CASES %lld ELEMENTS %lld ROWS %lld GROUPS %lld WORKSPACE %lld VIOLATIONS %lld\n", cases, elements, rows_total, groups_total,
           workspace_total, violations);
    return violations ? 1 : 0;
}
