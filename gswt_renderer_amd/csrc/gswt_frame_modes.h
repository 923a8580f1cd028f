// gswt_frame_modes.h -- the two pure rules behind the per-frame modes of the strict vertex stage (orthographic projection, pixel filter,
// atmosphere, tile styles, sun shadows, clip volumes): which k_project instantiation a frame's modes select, and which version of a versioned resource
// may be refilled.  Host-only and free of HIP (tools/frame_modes_main.cpp compiles it with the host compiler alone); gswt_ctx.h holds the
// records the rules read (FrameModes, VersionPool).
#pragma once

namespace gswt {

// The mode bits of k_project<DEBUG, FULL, STRICT, ORTHO, AA, ATM, STY, SHD, CLIP> (launch_project maps them onto with_variant as they stand).
struct ProjectModes { bool strict, ortho, aa, atm, sty, shd, clip; };

// THE rule, from what a frame kept from its submission (FrameModes, gswt_ctx.h; a template so that this header needs neither it nor Atmo).
// The orthographic stage exists in its strict form only, so an orthographic frame runs the strict sequence.  Every other mode is a
// parameter of the STRICT instantiations only: the v2 sequence has no such form, validate_frame_modes (gswt_api.hip) refuses such a frame,
// and a frame with a mode off launches the instantiation it always did.  On: the filter with aa_s > 0, the atmosphere with the far fade
// or the fog on, the styles and the shadows with a version of their table / map, the clip volumes with at least one volume in the set.
template <typename Modes>
constexpr ProjectModes project_modes(const Modes& m)
{
    const bool strict = m.strict_vs || m.ortho;
    return ProjectModes{strict, m.ortho, strict && m.aa_s > 0.0f, strict && (m.atm.fade_end > 0.0f || m.atm.fog_density > 0.0f),
                        strict && m.sty_ver >= 0, strict && m.shd_ver >= 0, strict && m.clip.n > 0u};
}

// A version of a resource that frames in flight keep their own version of: the lowest of n_versions that is neither the current one nor
// named by a frame slot (ver_of(slot); -1 names none).  -1: none is free, which n_versions >= the number of slots + 2 rules out.
template <typename Slots, typename VerOf>
constexpr int free_version(int n_versions, int cur, const Slots& slots, VerOf ver_of)
{
    for (int k = 0; k < n_versions; k++) {
        bool used = k == cur;
        for (const auto& sl : slots) used = used || ver_of(sl) == k;
        if (!used) return k;
    }
    return -1;
}

}  // namespace gswt
