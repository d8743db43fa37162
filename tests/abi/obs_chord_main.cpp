// Stand-alone driver of the observation kernel's chord selection (collision_avoidance_amd/csrc/ca_obs_chord.h): no device, no library.
// tests/test_obs_entry_chord_cpu.py compiles it for the host and runs it as a child process.
//
//   obs_chord_main <cases.f32> <out.i8>
//
// cases.f32: records of 8 floats -- the agent's frame (cos, sin), the neighbour's position relative to the agent (rx, ry), the
// radius R of the neighbour's octagon, the ray's end point (s10x, s10y) and the range (rays[0], for the tolerance).
// out.i8: 4 signed bytes per case -- the path (1: the entry chord alone, 0: every survivor), the chord that wins the pair (-1: no
// hit), the survivor mask, and the chord tested first.
// A case goes the way a lane of phase A's pair loop goes (ca_obs.h): obs_chord_cross and obs_chord_select are the header's, the
// chord's geometry, the accept test and the distance are the kernel's expressions (env.py:335-350, utils.py:14-38) in fp32 without
// fused operations (ca_math.h's host forms of the division and the square root).  Prints OBS_CHORD_OK and the counts at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ca_obs_chord.h"

struct Seg { float s02x, s02y, s32x, s32y, t_numer; };

static void build_nb(const float (&oct)[16], float fc, float fs, float rx, float ry, int e, Seg& sg) {
    const float x1 = oct[2 * e] + rx, y1 = oct[2 * e + 1] + ry, x2 = oct[2 * ((e + 1) & 7)] + rx, y2 = oct[2 * ((e + 1) & 7) + 1] + ry;
    const float r1x = fc * x1 - fs * y1, r1y = fs * x1 + fc * y1;  // utils.py:59
    const float r2x = fc * x2 - fs * y2, r2y = fs * x2 + fc * y2;  // utils.py:60
    sg.s32x = r2x - r1x; sg.s32y = r2y - r1y;
    sg.s02x = 0.0f - r1x; sg.s02y = 0.0f - r1y;
    sg.t_numer = sg.s32x * sg.s02y - sg.s32y * sg.s02x;
}

static bool accept_nb(const Seg& sg, float s10x, float s10y, float& denom) {
    denom = s10x * sg.s32y - sg.s32x * s10y;                      // utils.py:14
    const float s_numer = s10x * sg.s02y - s10y * sg.s02x;        // utils.py:21
    const bool dpos = denom > 0.0f;
    return (denom != 0.0f) && ((s_numer < 0.0f) != dpos) && ((sg.t_numer < 0.0f) != dpos) &&
           ((s_numer > denom) != dpos) && ((sg.t_numer > denom) != dpos);  // utils.py:15-31
}

static float hit_dist(float t_numer, float denom, float s10x, float s10y) {
    const float t = ca::div_ir(t_numer, denom);                    // utils.py:34
    const float hx = 0.0f + t * s10x, hy = 0.0f + t * s10y;        // utils.py:36-37
    return ca::sqrt_ir(hx * hx + hy * hy);                         // utils.py:38
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <cases.f32> <out.i8>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    std::vector<float> rec;
    {
        std::vector<float> buf(8 * 65536);
        size_t got;
        while ((got = std::fread(buf.data(), sizeof(float), buf.size(), in)) > 0) rec.insert(rec.end(), buf.begin(), buf.begin() + got);
    }
    std::fclose(in);
    if (rec.size() % 8 != 0) { std::fprintf(stderr, "%s: not a whole number of records\n", argv[1]); return 2; }
    const size_t n = rec.size() / 8;
    std::vector<signed char> out(4 * n);
    size_t nfast = 0, nslow = 0;
    float lastR = -1.0f, oct[16] = {0};
    for (size_t i = 0; i < n; ++i) {
        const float* c = &rec[8 * i];
        const float fc = c[0], fs = c[1], rx = c[2], ry = c[3], R = c[4], s10x = c[5], s10y = c[6], range = c[7];
        if (R != lastR) {   // vertex e = ((float)(R cos(e pi/4)), (float)(-(R sin(e pi/4)))) in fp64 from the fp32 radius
            for (int e = 0; e < 8; ++e) {
                const double th = e * (2.0 * M_PI / 8);
                oct[2 * e] = (float)((double)R * std::cos(th)); oct[2 * e + 1] = (float)(-((double)R * std::sin(th)));
            }
            lastR = R;
        }
        float cr[8];
        ca::obs_chord_cross(fc, fs, rx, ry, s10x, s10y, R, cr);
        const ca::ChordSel sel = ca::obs_chord_select(cr, ca::obs_chord_tol(range, R), rx * rx + ry * ry, R);
        float best = INFINITY;
        int best_e = -1;
        unsigned acc = sel.rest;
        int e1 = sel.first;
        bool todo = sel.acc != 0u;
        while (todo) {   // phase A's pair loop, for one lane
            Seg g1;
            build_nb(oct, fc, fs, rx, ry, e1, g1);
            float dn1;
            const bool ok1 = accept_nb(g1, s10x, s10y, dn1);
            const bool two = acc != 0u;
            if (!two) {
                const float dw = hit_dist(g1.t_numer, dn1, s10x, s10y);
                if (ok1 && dw < best) { best = dw; best_e = e1; }
                break;
            }
            const int e2 = __builtin_ffs((int)acc) - 1;
            acc &= acc - 1;
            Seg g2;
            build_nb(oct, fc, fs, rx, ry, e2, g2);
            float dn2;
            const bool ok2 = accept_nb(g2, s10x, s10y, dn2);
            const float lhs = std::fabs(g1.t_numer) * std::fabs(dn2), rhs = std::fabs(g2.t_numer) * std::fabs(dn1);
            const bool first = ok1 && (!ok2 || lhs < rhs);
            const float tnw = first ? g1.t_numer : g2.t_numer, dnw = first ? dn1 : dn2;
            const int ew = first ? e1 : e2;
            const bool sure = std::fmin(lhs, rhs) < 0.99999f * std::fmax(lhs, rhs) && std::fmax(lhs, rhs) > 1e-30f &&
                              std::fabs(tnw) > 1e-12f * std::fabs(dnw);
            if (ok1 && ok2 && !sure) {
                const float d1 = hit_dist(g1.t_numer, dn1, s10x, s10y), d2 = hit_dist(g2.t_numer, dn2, s10x, s10y);
                if (d1 < best) { best = d1; best_e = e1; }
                if (d2 < best) { best = d2; best_e = e2; }
            } else if (ok1 || ok2) {
                const float dw = hit_dist(tnw, dnw, s10x, s10y);
                if (dw < best) { best = dw; best_e = ew; }
            }
            todo = acc != 0u;
            e1 = __builtin_ffs((int)acc) - 1;
            acc &= acc - 1;
        }
        (sel.fast ? nfast : nslow) += 1;
        out[4 * i] = sel.fast ? 1 : 0;
        out[4 * i + 1] = (signed char)best_e;
        out[4 * i + 2] = (signed char)(unsigned char)sel.acc;
        out[4 * i + 3] = (signed char)sel.first;
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) { std::perror(argv[2]); return 2; }
    const bool wrote = std::fwrite(out.data(), 1, out.size(), fo) == out.size();
    if (std::fclose(fo) != 0 || !wrote) { std::fprintf(stderr, "%s: short write\n", argv[2]); return 2; }
    std::printf("OBS_CHORD_OK %zu cases: %zu fast, %zu slow\n", n, nfast, nslow);
    return 0;
}
