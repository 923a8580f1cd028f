// frame_modes_clip_main.cpp -- project_modes (gswt_frame_modes.h) with the clip volumes' count as its seventh input, as a stand-alone host
// program for tests/test_clip_cpu.py:
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror -I gswt_renderer_amd/csrc tools/frame_modes_clip_main.cpp -o frame_modes_clip
// Over all 128 inputs (strict_vs, ortho, filter on, atmosphere on, styles on, shadows on, volumes set -- by 1 and by 8 volumes): strict =
// strict_vs or ortho, every other mode = its input and strict, `clip` among them, and all 64 instantiations of the strict sequence are
// reached.  Prints one "FAIL ..." line per violated property (at most 20) and, last, "project_modes: N inputs, N strict outputs".
// Exit status 1 when anything failed.  (tools/frame_modes_main.cpp keeps the 64 inputs of a frame without volumes.)
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
    bool reached[64] = {};
    int n_inputs = 0;
    for (int in = 0; in < 128; in++) {
        const bool strict_vs = in & 1, ortho = in & 2, aa = in & 4, atm = in & 8, sty = in & 16, shd = in & 32, clip = in & 64;
        for (unsigned n_vol = clip ? 1u : 0u; n_vol <= (clip ? 8u : 0u); n_vol += 7u) {
            const Modes m = {strict_vs, ortho, aa ? 0.25f : 0.0f, {atm ? 100.0f : 0.0f, 0.0f}, sty ? 3 : -1, shd ? 0 : -1, {n_vol}};
            const gswt::ProjectModes p = gswt::project_modes(m);
            const bool strict = strict_vs || ortho;
            CHECK(p.strict == strict, "project_modes input %d", in);
            CHECK(p.ortho == ortho, "project_modes input %d", in);
            CHECK(p.aa == (aa && strict), "project_modes input %d", in);
            CHECK(p.atm == (atm && strict), "project_modes input %d", in);
            CHECK(p.sty == (sty && strict), "project_modes input %d", in);
            CHECK(p.shd == (shd && strict), "project_modes input %d", in);
            CHECK(p.clip == (clip && strict), "project_modes input %d (%u volumes)", in, n_vol);
            if (p.strict) reached[p.ortho | p.aa << 1 | p.atm << 2 | p.sty << 3 | p.shd << 4 | p.clip << 5] = true;
        }
        n_inputs++;
    }
    int n_reached = 0;
    for (bool r : reached) n_reached += r;
    CHECK(n_reached == 64, "project_modes reaches %d strict outputs", n_reached);
    std::printf("project_modes: %d inputs, %d strict outputs\n", n_inputs, n_reached);
    return n_failed ? 1 : 0;
}
