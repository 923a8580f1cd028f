// with_variant_main.cpp -- gswt_variant.h's with_variant / OneOf (the one way a launch wrapper picks a kernel instantiation) as a stand-alone
// host program, for tests/test_with_variant_cpu.py:
//   g++ -std=c++17 -O1 -Wall -Wextra -I gswt_renderer_amd/csrc tools/with_variant_main.cpp -o with_variant
// For three bool selectors and one OneOf<0, 1, 2>, in the order (bool, bool, OneOf, bool), it calls with_variant with every combination of
// runtime values -- the OneOf also with the out-of-list values -1, 3 and 7 -- and prints one line per call of the lambda:
//   "in a b v c -> A B V C"   (runtime selectors, then the compile-time constants the lambda received, in its parameter order)
// A call that does not reach the lambda prints nothing; one that reaches it twice prints two lines.  The constants are used as template
// arguments, as a launch wrapper uses them.
#include <cstdio>

#include "gswt_variant.h"

template <bool A, bool B, int V, bool C>
static void landed(bool a, bool b, int v, bool c)
{
    std::printf("in %d %d %d %d -> %d %d %d %d\n", (int)a, (int)b, v, (int)c, (int)A, (int)B, V, (int)C);
}

int main()
{
    const int vs[] = {0, 1, 2, -1, 3, 7};
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++)
            for (int v : vs)
                for (int c = 0; c < 2; c++)
                    gswt::with_variant([&](auto A, auto B, auto V, auto C) { landed<A, B, V, C>(a != 0, b != 0, v, c != 0); }, a != 0, b != 0,
                                       gswt::OneOf<0, 1, 2>{v}, c != 0);
    // no selector: the lambda runs once
    gswt::with_variant([] { std::printf("in -> \n"); });
    return 0;
}
