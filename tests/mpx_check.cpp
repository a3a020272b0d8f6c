// mpx_check.cpp -- the multiplex spectrum meter's pure functions (sdr-j-fm_amd/csrc/fmx_mpx.h), the grid it takes from fmx_spec.h and the survey's stage
// functions (fmx_survey.h) compiled for the host and driven as fmx_mpx.hip and stage_mpx drive them: piece by piece, launch by launch (spec::launches),
// thread by thread, pass by pass, with one LDS image, one carry, one sum and one maximum per bin and a ring of four records.  tests/test_mpx_cpu.py sets
// the result ("kernel_form") against the float64 model of tests/mpx_model.py.
//
//   mpx_check spectrum in.f32 out.f32 B S on_call scratch_blocks [piece lengths ...]
//       in: one channel's demodulator output as f32 from fm sample 0, cut into pieces of the given lengths (none: one piece); the meter is switched on by
//       piece `on_call` (0: from the start).  The scratch holds scratch_blocks blocks of 2048 powers.  out: one row of 1 + 2 * 2048 f32 per record
//       delivered, written behind the piece that completed it if it was still in the ring: index, mean, peak.
//   mpx_check defect <kind> in.f32 out.f32 B S on_call scratch_blocks [piece lengths ...]
//       the same run with one defect seeded into THIS DRIVER's use of the header, for the detector's test (tests/test_mpx_cpu.py):
//       kind 1: a stale carry sample -- the carry write skips position 700; 2: the row is read one sample late in the second piece;
//       3: a block left out -- block 3's powers do not reach the fold (they read zero)
//   mpx_check plan g0 n S B [...]
//       prints spec::piece's answer for every four numbers: b0 blocks fill fill_after append carry_src phase record0 records
//   mpx_check launches channels blocks carries [...]
//       prints spec::launches' visits with the meter's own scratch (mpx::SCRATCH_BLOCKS) for every three numbers, `j0 gn done nb write_carry`, then `end`
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdr-j-fm_amd/csrc/fmx_mpx.h"

using namespace fmx;

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) {
        for (int a = 2; a + 3 < argc; a += 4) {
            const spec::Piece p = spec::piece(std::atoll(argv[a]), std::atoll(argv[a + 1]), (int32_t)std::atoi(argv[a + 2]), (int32_t)std::atoi(argv[a + 3]));
            std::printf("%lld %lld %d %d %d %lld %d %lld %lld\n", (long long)p.b0, (long long)p.blocks, (int)p.fill, (int)p.fill_after, (int)p.append,
                        (long long)p.carry_src, (int)p.phase, (long long)p.record0, (long long)p.records);
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "launches")) {
        for (int a = 2; a + 2 < argc; a += 3) {
            spec::launches(std::atoll(argv[a]), mpx::SCRATCH_BLOCKS, std::atoll(argv[a + 1]), std::atoi(argv[a + 2]) != 0,
                           [](int64_t j0, int64_t gn, int64_t done, int64_t nb, bool wc) {
                               std::printf("%lld %lld %lld %lld %d\n", (long long)j0, (long long)gn, (long long)done, (long long)nb, wc ? 1 : 0);
                           });
            std::printf("end\n");
        }
        return 0;
    }
    int defect = 0;
    if (argc >= 3 && !std::strcmp(argv[1], "defect")) {          // (drop the kind: the rest is spectrum's command line)
        defect = std::atoi(argv[2]);
        static char name[] = "spectrum";
        argv[2] = name; argv++; argc--;
    }
    if (argc < 8 || std::strcmp(argv[1], "spectrum")) { std::fprintf(stderr, "usage: see the head of mpx_check.cpp\n"); return 2; }
    FILE *fi = std::fopen(argv[2], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); const long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    std::vector<float> in((size_t)bytes / sizeof(float));
    if (std::fread(in.data(), sizeof(float), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);
    const int B = std::atoi(argv[4]), S = std::atoi(argv[5]), on_call = std::atoi(argv[6]);
    const int64_t scratch = std::atoll(argv[7]);
    if (B < 1 || B > mpx::MAX_B || S < 1 || S > mpx::MAX_S || scratch < 1) return 2;
    std::vector<int64_t> calls;
    int64_t sum = 0;
    for (int a = 8; a < argc; a++) { calls.push_back(std::atoll(argv[a])); sum += calls.back(); }
    if (calls.empty()) calls.push_back((int64_t)in.size());
    else if (sum != (int64_t)in.size()) return 2;

    std::vector<float> window(mpx::N), carry(mpx::N, 0.f);
    std::vector<float2> W(mpx::N), lds(survey::LDS_N), regs((size_t)mpx::NT * mpx::PER);
    survey::make_window(window.data());
    survey::make_twiddles(W.data());
    const float c = survey::record_scale(window.data(), B), c1 = survey::record_scale(window.data(), 1);
    std::vector<float> acc((size_t)2 * mpx::BINS, 0.f), ring((size_t)mpx::RING * 2 * mpx::BINS, 0.f), power((size_t)scratch * mpx::BINS);
    FILE *fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    int64_t g0 = 0, on_from = -1;
    int k = 0;
    for (const int64_t n : calls) {
        const float *row = in.data() + g0 + ((defect == 2 && k == 1 && g0 + n < (int64_t)in.size()) ? 1 : 0);          // (the row of a piece holds that piece's fm samples only)
        if (k++ >= on_call) {
            if (on_from < 0) on_from = g0;
            const int64_t first = spec::first_block(on_from, S);
            const spec::Piece p = spec::piece(g0, n, S, B);
            spec::launches(1, scratch, p.blocks, p.fill_after > 0, [&](int64_t, int64_t, int64_t done, int64_t nb, bool write_carry) {
                for (int64_t j = 0; j < nb; j++) {                             // mpx_block_kernel, workgroup j of the chunk
                    const int64_t b = p.b0 + done + j;
                    for (int t = 0; t < mpx::NT; t++) {
                        float2 x[mpx::PER];
                        for (int n2 = 0; n2 < mpx::PER; n2++) if (spec::source_index(b, t + 256 * n2, g0, S) >= n) std::abort();      // (the block completes in the piece)
                        mpx::load(t, b, g0, n, S, carry.data(), row, window.data(), x);
                        survey::pass1(t, x, W.data(), lds.data());
                    }
                    for (int t = 0; t < mpx::NT; t++) survey::pass2_load(t, lds.data(), &regs[(size_t)t * mpx::PER]);
                    for (int t = 0; t < mpx::NT; t++) survey::pass2_store(t, &regs[(size_t)t * mpx::PER], W.data(), lds.data());
                    for (int t = 0; t < mpx::NT; t++) {
                        float pw[mpx::PER];
                        survey::pass3(t, lds.data(), W.data(), pw);
                        for (int cc = 0; cc < mpx::KEEP; cc++) power[(size_t)j * mpx::BINS + t + 256 * cc] = (defect == 3 && b == 3) ? 0.f : pw[cc];
                    }
                }
                for (int i = 0; i < mpx::N; i++) {                             // mpx_fold_kernel, thread i
                    if (nb > 0 && i < mpx::BINS)
                        mpx::fold(acc[i], acc[mpx::BINS + i], power.data() + i, mpx::BINS, p.b0 + done, nb, first, (int)((p.b0 + done) % B), B, c, c1,
                                  ring.data() + i, ring.data() + mpx::BINS + i);
                    if (!write_carry || (defect == 1 && i == 700)) continue;
                    if (p.append) { if (i < n) carry[(size_t)(p.fill + i)] = row[i]; }
                    else if (i < p.fill_after) carry[i] = row[p.carry_src + i];
                }
            });
            const int64_t r_end = p.record0 + p.records;
            for (int64_t r = std::max(p.record0, r_end - mpx::RING); r < r_end; r++) {
                if (!spec::delivered(r, B, first)) continue;
                const float index = (float)r;
                std::fwrite(&index, sizeof(float), 1, fo);
                std::fwrite(ring.data() + (size_t)(r % mpx::RING) * 2 * mpx::BINS, sizeof(float), (size_t)2 * mpx::BINS, fo);
            }
        }
        g0 += n;
    }
    std::fclose(fo);
    return 0;
}
