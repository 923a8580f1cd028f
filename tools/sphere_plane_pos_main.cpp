// sphere_plane_pos_main.cpp -- host/gswt_surface.h's sphere_plane_pos (the inverse of the sphere unfolding k_proxy_sphere textures through)
// as a stand-alone host program, for tests/test_proxy_sphere_cpu.py: built with the compiler's address and undefined-behaviour sanitizers,
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I gswt_renderer_amd/csrc tools/sphere_plane_pos_main.cpp -o sphere_plane_pos
// Reads lines "block_w nx ny nz" from standard input and prints "px py" of each (%.9g: a binary32 value survives the round trip).
#include <cstdio>

#include "host/gswt_surface.h"

int main()
{
    float bw, x, y, z;
    while (std::scanf("%f %f %f %f", &bw, &x, &y, &z) == 4) {
        float px = 0.0f, py = 0.0f;
        gswt_host::sphere_plane_pos(bw, gswt_host::V3{x, y, z}, px, py);
        std::printf("%.9g %.9g\n", px, py);
    }
    return 0;
}
