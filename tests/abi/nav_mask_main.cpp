// The navigation grid's mask builder (csrc/ca_nav_host.h) as a stand-alone program: tests/test_nav_cpu.py compiles it with
// -fsanitize=address,undefined and runs it.  Every mask goes into a heap buffer of exactly gx * gy bytes, so a write past the grid is
// an error the sanitizer reports; the masks are checked against the definition evaluated cell by cell, edge by edge.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ca_nav_host.h"

static void rect(std::vector<float>& e, float x0, float y0, float x1, float y1) {
    const float v[4][2] = {{x0, y0}, {x1, y0}, {x1, y1}, {x0, y1}};
    for (int i = 0; i < 4; ++i) {
        e.push_back(v[i][0]); e.push_back(v[i][1]); e.push_back(v[(i + 1) % 4][0]); e.push_back(v[(i + 1) % 4][1]);
    }
}

static int check(const char* name, const std::vector<float>& e, float x0, float y0, float cs, int gx, int gy, float clearance) {
    const int n = (int)(e.size() / 4);
    uint8_t* got = (uint8_t*)malloc((size_t)gx * gy);
    ca_nav::mask_build(e.data(), n, x0, y0, cs, gx, gy, clearance, got);
    int bad = 0, blocked = 0;
    for (int cy = 0; cy < gy; ++cy)
        for (int cx = 0; cx < gx; ++cx) {
            bool b = false;
            for (int k = 0; k < n; ++k)
                if (ca_nav::dist_sq_point_segment(e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3], ca_nav::centre(x0, cx, cs), ca_nav::centre(y0, cy, cs)) <
                    clearance * clearance)
                    b = true;
            bad += (got[cy * gx + cx] != 0) != b;
            blocked += b;
        }
    free(got);
    printf("%s: %d x %d cells, %d edges, %d blocked, %d wrong\n", name, gx, gy, n, blocked, bad);
    return bad;
}

int main() {
    int bad = 0;
    std::vector<float> door, blocks, hall, none;
    rect(door, -15.0f, 0.0f, 10.0f, 10.0f); rect(door, 2.0f, 0.0f, 2.5f, 4.4f); rect(door, 2.0f, 5.6f, 2.5f, 10.0f);
    rect(blocks, 1.5f, 1.5f, 2.5f, 2.5f); rect(blocks, 5.0f, 1.5f, 6.0f, 2.5f); rect(blocks, 1.5f, 5.0f, 2.5f, 6.0f); rect(blocks, 4.5f, 4.5f, 5.5f, 5.5f);
    rect(hall, 0.0f, 0.0f, 64.0f, 32.0f);
    bad += check("doorway", door, -2.0f, 0.0f, 1.0f, 12, 10, 0.05f);
    bad += check("doorway, clearance = the distance of a centre", door, -2.0f, 0.0f, 1.0f, 12, 10, 0.5f);
    bad += check("blocks", blocks, 0.0f, 0.0f, 1.0f, 8, 8, 0.3f);
    bad += check("one cell", blocks, 1.6f, 1.6f, 1.0f, 1, 1, 0.3f);
    bad += check("hall", hall, 0.0f, 0.0f, 0.25f, 256, 128, 0.3f);
    bad += check("grid beside the world", door, 40.0f, 40.0f, 0.5f, 13, 7, 0.5f);
    bad += check("grid inside one wall's reach", door, 1.9f, 1.0f, 0.01f, 40, 40, 1000.0f);
    bad += check("no edges", none, 0.0f, 0.0f, 1.0f, 5, 5, 0.5f);
    bad += check("no clearance", door, -2.0f, 0.0f, 1.0f, 12, 10, 0.0f);
    bad += check("far from the origin", door, -9.0e4f, 9.0e4f, 1.0e-3f, 16, 16, 1.0e-3f);
    if (bad) { printf("NAV_MASK_BAD %d\n", bad); return 1; }
    printf("NAV_MASK_OK\n");
    return 0;
}
