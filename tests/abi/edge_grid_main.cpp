// Stand-alone driver of the static edge grid's host builder (collision_avoidance_amd/csrc/ca_edge_grid_host.h): no HIP, no library.
// tests/test_edge_grid_cpu.py compiles it with -fsanitize=address,undefined and runs it as a child process.  It builds sets of the
// kinds the python test builds (pillars, an enclosing box, long diagonals, a world translated by 5e4 with 500-long edges, a single
// edge, edges on one line, no edge at all), checks each table's CSR invariants, walks it from seeded points the way the kernels do
// and checks that no edge is taken twice, and provokes both refusals.  Prints EDGE_GRID_OK and returns 0 when everything held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ca_edge_grid_host.h"

namespace eg = ca_edge_grid;

static unsigned long long g_state = 88172645463325252ull;
static double uni(double lo, double hi) {   // xorshift64: seeded, the same everywhere
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return lo + (hi - lo) * (double)(g_state >> 11) / 9007199254740992.0;
}

static void add_box(std::vector<float>& e, double x0, double y0, double x1, double y1) {
    const double v[4][2] = {{x0, y0}, {x0, y1}, {x1, y1}, {x1, y0}};
    for (int i = 0; i < 4; ++i) { e.push_back((float)v[i][0]); e.push_back((float)v[i][1]); e.push_back((float)v[(i + 1) & 3][0]); e.push_back((float)v[(i + 1) & 3][1]); }
}

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s: %s (line %d)\n", name, #c, __LINE__); return 1; } } while (0)

static int check_set(const char* name, const std::vector<float>& e, float range) {
    const int n = (int)(e.size() / 4);
    eg::Desc d0, d;
    std::vector<uint32_t> cs, en;
    REQUIRE(eg::build(e.data(), n, range, d0, nullptr, nullptr) == eg::OK);
    REQUIRE(eg::build(e.data(), n, range, d, &cs, &en) == eg::OK);
    REQUIRE(d0.gx == d.gx && d0.gy == d.gy && d0.n_entries == d.n_entries);
    REQUIRE(d.gx >= 1 && d.gx <= eg::MAX_SIDE && d.gy >= 1 && d.gy <= eg::MAX_SIDE);
    REQUIRE(cs.size() == (size_t)d.gx * d.gy + 1 && en.size() == (size_t)d.n_entries && cs[0] == 0u && cs.back() == (uint32_t)d.n_entries);
    for (size_t c = 0; c + 1 < cs.size(); ++c) REQUIRE(cs[c] <= cs[c + 1]);
    for (uint32_t w : en) REQUIRE((int)(w & 0xFFFFu) < n && (int)((w >> 16) & 0xFFu) < d.gx && (int)(w >> 24) < d.gy);
    std::vector<int> seen((size_t)n + 1, -1);
    double lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0};
    for (int k = 0; k < 4 * n; ++k) { if (k < 2 || e[k] < lo[k & 1]) lo[k & 1] = e[k]; if (k < 2 || e[k] > hi[k & 1]) hi[k & 1] = e[k]; }
    for (int p = 0; p < 4000; ++p) {
        const float x = (float)uni(lo[0] - 60.0, hi[0] + 60.0), y = (float)uni(lo[1] - 60.0, hi[1] + 60.0);
        const int cxlo = eg::cell(x - range, d.x0, d.ics_x, d.gx), cxhi = eg::cell(x + range, d.x0, d.ics_x, d.gx);
        const int cylo = eg::cell(y - range, d.y0, d.ics_y, d.gy), cyhi = eg::cell(y + range, d.y0, d.ics_y, d.gy);
        REQUIRE(cxlo <= cxhi && cylo <= cyhi && cxhi - cxlo <= 3 && cyhi - cylo <= 3);
        for (int r = cylo; r <= cyhi; ++r)
            for (int c = cxlo; c <= cxhi; ++c)
                for (uint32_t u = cs[(size_t)r * d.gx + c]; u < cs[(size_t)r * d.gx + c + 1]; ++u) {
                    const uint32_t w = en[u];
                    const int ec = (int)((w >> 16) & 0xFFu), er = (int)(w >> 24);
                    if ((ec > cxlo ? ec : cxlo) != c || (er > cylo ? er : cylo) != r) continue;
                    REQUIRE(seen[w & 0xFFFFu] != p);   // no edge twice
                    seen[w & 0xFFFFu] = p;
                }
    }
    std::printf("%-12s %6d edges  %3d x %3d cells  %8d entries  margin %g\n", name, n, (int)d.gx, (int)d.gy, (int)d.n_entries, (double)d.margin);
    return 0;
}

int main() {
    int bad = 0;
    std::vector<float> e;
    for (int y = 0; y < 11; ++y) for (int x = 0; x < 11; ++x) add_box(e, 1.25 + 3 * x, 1.25 + 3 * y, 1.75 + 3 * x, 1.75 + 3 * y);
    bad += check_set("pillars", e, 2.0f);
    add_box(e, 0.0, 0.0, 34.641, 34.641);
    bad += check_set("hall", e, 2.0f);
    e.clear();
    for (int k = 0; k < 12; ++k) { e.push_back((float)uni(-20, 70)); e.push_back((float)uni(10, 100)); e.push_back((float)uni(-20, 70)); e.push_back((float)uni(10, 100)); }
    bad += check_set("diagonals", e, 2.0f);
    e.clear();
    add_box(e, 5e4, -5e4, 5e4 + 500.0, -5e4 + 500.0);
    for (int k = 0; k < 40; ++k) { const double x = 5e4 + uni(5, 490), y = -5e4 + uni(5, 490); add_box(e, x, y, x + 0.5, y + 0.5); }
    bad += check_set("translated", e, 2.0f);
    e.assign({1.0f, 2.0f, 4.5f, 3.25f});
    bad += check_set("single", e, 2.0f);
    e.clear();
    for (int k = 0; k < 24; ++k) { e.push_back(2.5f * k); e.push_back(3.0f); e.push_back(2.5f * k + (float)uni(0.5, 2.4)); e.push_back(3.0f); }
    bad += check_set("one_line", e, 1.3f);
    e.clear();
    bad += check_set("empty", e, 2.0f);

    const char* name = "refusals";
    eg::Desc d;
    std::vector<uint32_t> cs, en;
    e.assign((size_t)4 * 65536, 0.0f);
    for (size_t k = 0; k < 65536; ++k) { e[4 * k] = (float)k; e[4 * k + 2] = (float)k + 0.5f; }
    REQUIRE(eg::build(e.data(), 65536, 2.0f, d, &cs, &en) == eg::TOO_MANY_EDGES && cs.empty() && en.empty());
    e.clear();
    for (int k = 0; k < 100; ++k) { e.push_back(0.0f + k); e.push_back(0.0f); e.push_back(6000.0f + k); e.push_back(6000.0f); }
    REQUIRE(eg::build(e.data(), 100, 2.0f, d, &cs, &en) == eg::TOO_MANY_ENTRIES && d.n_entries > eg::MAX_ENTRIES && cs.empty());
    REQUIRE(eg::build(e.data(), 100, 0.0f, d, &cs, &en) == eg::BAD_RANGE);
    if (bad) return 1;
    std::printf("EDGE_GRID_OK\n");
    return 0;
}
