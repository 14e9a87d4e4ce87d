// Host check of csrc/fdc_math.h's packed wave sums (wave_sum64_pack_w on WaveModel, the sixty-four-lane model of the DPP moves) against
// wave_sum64's own moves on the same model, value by value.  Stand-alone program (its own main), built with
// -fsanitize=address,undefined by tests/test_wave_sum_pack_cpu.py.
//   stdin:  per case a line "N" and a line of 64 N hex words, lane-major ([64][N])
//   stdout: per case three lines of N hex words: the packed tree, wave_sum64, and a MUTANT of wave_sum64 that adds the rows pairwise,
//           (r0 + r1) + (r2 + r3) -- what the inputs must be able to tell apart
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fdc_math.h"

using fdc::WaveModel;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float flt(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static float mutant_sum(WaveModel v) {
    typedef WaveModel W;
    v = W::add(v, W::dpp<0xB1>(W::zero(), v));
    v = W::add(v, W::dpp<0x4E>(W::zero(), v));
    v = W::add(v, W::dpp<0x141>(W::zero(), v));
    v = W::add(v, W::dpp<0x140>(W::zero(), v));
    return (v.x[0] + v.x[16]) + (v.x[32] + v.x[48]);
}

template <int N>
static void run(const std::vector<uint32_t>& in) {
    WaveModel v[N];
    for (int l = 0; l < 64; ++l)
        for (int i = 0; i < N; ++i) v[i].x[l] = flt(in[(size_t)l * N + i]);
    const WaveModel r = fdc::wave_sum64_pack_w<WaveModel, N>(v, 0);
    for (int i = 0; i < N; ++i) printf("%08x%c", bits(r.x[fdc::WAVE_PACK_LANE0 + i]), i + 1 < N ? ' ' : '\n');
    for (int i = 0; i < N; ++i) printf("%08x%c", bits(fdc::wave_sum64_model(v[i])), i + 1 < N ? ' ' : '\n');
    for (int i = 0; i < N; ++i) printf("%08x%c", bits(mutant_sum(v[i])), i + 1 < N ? ' ' : '\n');
}

int main() {
    int n;
    while (scanf("%d", &n) == 1) {
        if (n < 1 || n > 16) return 2;
        std::vector<uint32_t> in((size_t)64 * n);
        for (auto& w : in)
            if (scanf("%x", &w) != 1) return 3;
        switch (n) {
        case 1: run<1>(in); break;
        case 2: run<2>(in); break;
        case 3: run<3>(in); break;
        case 4: run<4>(in); break;
        case 5: run<5>(in); break;
        case 6: run<6>(in); break;
        case 7: run<7>(in); break;
        case 8: run<8>(in); break;
        case 9: run<9>(in); break;
        case 10: run<10>(in); break;
        case 11: run<11>(in); break;
        case 12: run<12>(in); break;
        case 13: run<13>(in); break;
        case 14: run<14>(in); break;
        case 15: run<15>(in); break;
        default: run<16>(in); break;
        }
    }
    return 0;
}
