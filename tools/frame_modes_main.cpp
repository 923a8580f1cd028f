// frame_modes_main.cpp -- gswt_frame_modes.h's two pure rules (which k_project instantiation a frame's modes select; which version of a
// versioned resource may be refilled) as a stand-alone host program, for tests/test_frame_mode_rules_cpu.py:
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror -I gswt_renderer_amd/csrc tools/frame_modes_main.cpp -o frame_modes
// Exhaustive over both rules' inputs; prints one "FAIL ..." line per violated property (at most 20) and, last, "free_version: N states"
// and "project_modes: N inputs, N strict outputs".  Exit status 1 when anything failed.  The clip volumes' count is held at 0 here: these are
// the 64 inputs and 32 instantiations of a frame without volumes; tools/frame_modes_clip_main.cpp checks the rule with the count as a seventh input.
#include <cstdio>

#include "gswt_frame_modes.h"

// the members project_modes reads, as FrameModes (gswt_ctx.h) names them
struct Modes {
    bool strict_vs, ortho;
    float aa_s;
    struct { float fade_end, fog_density; } atm;
    int sty_ver, shd_ver;
    struct { unsigned n; } clip;
};

static int n_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond) && n_failed++ < 20) { std::printf("FAIL " __VA_ARGS__); std::printf(": %s\n", #cond); } \
    } while (0)

int main()
{
    // ---- free_version: five frame slots, N = 7 versions; cur and every slot's version in -1 .. N - 1
    constexpr int kSlots = 5, kVersions = kSlots + 2, kValues = kVersions + 1;
    long n_states = 0;
    int cur = -1, slot_ver[kSlots];
    for (long code = 0; code < 262144; code++) {              // 8^6
        long q = code;
        cur = (int)(q % kValues) - 1;
        for (int& x : slot_ver) { q /= kValues; x = (int)(q % kValues) - 1; }
        const int v = gswt::free_version(kVersions, cur, slot_ver, [](int ver) { return ver; });
        auto used = [&](int k) { bool u = k == cur; for (int i = 0; i < kSlots; i++) u = u || slot_ver[i] == k; return u; };
        CHECK(v >= 0 && v < kVersions, "free_version state %ld -> %d", code, v);
        if (v < 0 || v >= kVersions) continue;
        CHECK(!used(v), "free_version state %ld -> %d", code, v);
        for (int k = 0; k < v; k++) CHECK(used(k), "free_version state %ld -> %d, but %d is free", code, v, k);
        n_states++;
    }
    static_assert(kValues * kValues * kValues * kValues * kValues * kValues == 262144, "8^6 states");

    // ---- project_modes: (strict_vs, ortho, aa on, atmosphere on, styles on, shadow on); the atmosphere is on by the fade, the fog or both
    bool reached[32] = {};
    int n_inputs = 0;
    for (int in = 0; in < 64; in++) {
        const bool strict_vs = in & 1, ortho = in & 2, aa = in & 4, atm = in & 8, sty = in & 16, shd = in & 32;
        for (int how = 1; how <= (atm ? 3 : 1); how++) {
            Modes m = {strict_vs, ortho, aa ? 0.25f : 0.0f, {0.0f, 0.0f}, sty ? 3 : -1, shd ? 0 : -1, {0u}};
            if (atm && (how & 1)) m.atm.fade_end = 100.0f;
            if (atm && (how & 2)) m.atm.fog_density = 0.5f;
            const gswt::ProjectModes p = gswt::project_modes(m);
            const bool strict = strict_vs || ortho;
            CHECK(p.strict == strict, "project_modes input %d", in);
            CHECK(p.ortho == ortho, "project_modes input %d", in);
            CHECK(p.aa == (aa && strict), "project_modes input %d", in);
            CHECK(p.atm == (atm && strict), "project_modes input %d (atmosphere by %d)", in, how);
            CHECK(p.sty == (sty && strict), "project_modes input %d", in);
            CHECK(p.shd == (shd && strict), "project_modes input %d", in);
            CHECK(!p.clip, "project_modes input %d", in);
            if (p.strict) reached[p.ortho | p.aa << 1 | p.atm << 2 | p.sty << 3 | p.shd << 4] = true;
        }
        n_inputs++;
    }
    int n_reached = 0;
    for (bool r : reached) n_reached += r;
    CHECK(n_reached == 32, "project_modes reaches %d strict outputs", n_reached);

    std::printf("free_version: %ld states\n", n_states);
    std::printf("project_modes: %d inputs, %d strict outputs\n", n_inputs, n_reached);
    return n_failed ? 1 : 0;
}
