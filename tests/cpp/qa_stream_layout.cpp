// The LDS layouts that the plans of k_resamp and k_arb choose (newsched_amd/csrc/nsh_stream_layout.hpp),
// printed one line per case for tests/test_stream_layout.py, which compares them with the Python
// models of tests/. Host arithmetic only: no device, no library call.
//
//   qa_stream_layout resamp I D [I D ...]   ->  resamp I D R linear G a
//   qa_stream_layout arb F s [F s ...]      ->  arb F s linear a pad      (step = s 2^27)
//   qa_stream_layout                        ->  a built-in list of both
#include "../../newsched_amd/csrc/nsh_stream_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static void resamp(int I, int D)
{
    const nsh::resamp_layout g = nsh::resamp_layout_of(I, D);
    std::printf("resamp %d %d %d %d %d %d\n", I, D, g.R, g.linear ? 1 : 0, g.G, g.a);
}

static int arb(int F, long long s)
{
    int fshift = 0;
    while ((1 << fshift) < F) ++fshift;
    if (fshift < 1 || fshift > 6 || (1 << fshift) != F || s < F / 2 || s > 2048ll * F) return 1;
    const nsh::arb_layout g = nsh::arb_layout_of((uint64_t)s << 27, fshift);
    std::printf("arb %d %lld %d %d %d\n", F, s, g.linear ? 1 : 0, g.a, g.pad);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 1) {
        const int v[] = { 1, 2, 3, 5, 7, 16, 31, 48, 63, 64 };
        for (int I : v)
            for (int D : v) resamp(I, D);
        for (int F : { 2, 4, 32, 64 })
            for (long long s : { F / 2ll, 32ll * F, 32ll * F + 1, 100ll * F + 3, 2048ll * F }) arb(F, s);
        return 0;
    }
    const bool is_resamp = !std::strcmp(argv[1], "resamp");
    if ((!is_resamp && std::strcmp(argv[1], "arb")) || argc % 2) {
        std::fprintf(stderr, "usage: %s [resamp I D ... | arb F s ...]\n", argv[0]);
        return 2;
    }
    for (int i = 2; i + 1 < argc; i += 2) {
        const long long x = std::atoll(argv[i]), y = std::atoll(argv[i + 1]);
        if (is_resamp) {
            if (x < 1 || x > 64 || y < 1 || y > 64) return 1;
            resamp((int)x, (int)y);
        } else if (arb((int)x, y))
            return 1;
    }
    return 0;
}
