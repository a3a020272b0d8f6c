// survey_check.cpp -- the band survey's stage functions (sdr-j-fm_amd/csrc/fmx_survey.h) compiled for the host and driven as the kernels of
// fmx_survey.hip drive them: thread by thread, pass by pass, with a barrier's place between the passes, one LDS image, one carry, one
// accumulator and a ring of four records.  tests/test_survey_cpu.py sets the result ("kernel_form") against a float64 model.
//
//   survey_check spectrum in.c64 out.f32 B [call lengths ...]
//       in: one stream of complex f32 samples, cut into calls of the given lengths (none: one call).  out: one row of 1 + 4096 f32 per record
//       that was still in the ring behind the call that completed it: the record's index, then P [0 .. 4095].
//   survey_check plan fill n_wide blocks_so_far B [...]
//       prints survey::plan's answer for every four numbers: blocks fill phase record0 records
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdr-j-fm_amd/csrc/fmx_survey.h"

using namespace fmx;

static int run_plan(int argc, char **argv) {
    for (int a = 2; a + 3 < argc; a += 4) {
        const survey::Plan p = survey::plan((int32_t)std::atoi(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), (int32_t)std::atoi(argv[a + 3]));
        std::printf("%lld %d %d %lld %lld\n", (long long)p.blocks, (int)p.fill, (int)p.phase, (long long)p.record0, (long long)p.records);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return run_plan(argc, argv);
    if (argc < 5 || std::strcmp(argv[1], "spectrum")) { std::fprintf(stderr, "usage: see the head of survey_check.cpp\n"); return 2; }
    FILE *fi = std::fopen(argv[2], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); const long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    std::vector<float2> in((size_t)bytes / sizeof(float2));
    if (std::fread(in.data(), sizeof(float2), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);
    const int B = std::atoi(argv[4]);
    if (B < 1 || B > survey::MAX_B) return 2;
    std::vector<int64_t> calls;
    int64_t sum = 0;
    for (int a = 5; a < argc; a++) { calls.push_back(std::atoll(argv[a])); sum += calls.back(); }
    if (calls.empty()) calls.push_back((int64_t)in.size());
    else if (sum != (int64_t)in.size()) return 2;

    std::vector<float> window(survey::N);
    std::vector<float2> W(survey::N), carry(survey::N), lds(survey::LDS_N), regs((size_t)survey::NT * survey::PER);
    survey::make_window(window.data());
    survey::make_twiddles(W.data());
    const float scale = survey::record_scale(window.data(), B);
    std::vector<float> acc(survey::N, 0.f), ring((size_t)survey::RING * survey::N, 0.f), power;
    FILE *fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    int32_t fill = 0;
    int64_t blocks = 0, pos = 0;
    for (const int64_t n_wide : calls) {
        const float2 *src = in.data() + pos;
        const survey::Plan p = survey::plan(fill, n_wide, blocks, B);
        power.assign((size_t)(p.blocks > 0 ? p.blocks : 1) * survey::N, 0.f);          // (never empty: the fold takes its address)
        for (int64_t j = 0; j < p.blocks; j++) {                         // survey_block_kernel, workgroup j
            for (int t = 0; t < survey::NT; t++) {
                float2 x[survey::PER];
                for (int n2 = 0; n2 < survey::PER; n2++) {
                    const int i = t + 256 * n2;
                    const int64_t q = survey::source_index(j, i, fill);
                    const float2 v = q < 0 ? carry[(size_t)(fill + q)] : src[q];
                    x[n2] = make_float2(v.x * window[i], v.y * window[i]);
                }
                survey::pass1(t, x, W.data(), lds.data());
            }
            for (int t = 0; t < survey::NT; t++) survey::pass2_load(t, lds.data(), &regs[(size_t)t * survey::PER]);
            for (int t = 0; t < survey::NT; t++) survey::pass2_store(t, &regs[(size_t)t * survey::PER], W.data(), lds.data());
            for (int t = 0; t < survey::NT; t++) {
                float pw[survey::PER];
                survey::pass3(t, lds.data(), W.data(), pw);
                for (int c = 0; c < survey::PER; c++) power[(size_t)j * survey::N + t + 256 * c] = pw[c];
            }
        }
        for (int i = 0; i < survey::N; i++) {                           // survey_fold_kernel, thread i
            acc[i] = survey::accumulate(acc[i], power.data() + i, p.blocks, p.phase, B, scale, ring.data() + i, (int)(p.record0 % survey::RING));
            if (p.blocks == 0) { if (i < n_wide) carry[(size_t)(fill + i)] = src[i]; }
            else if (i < p.fill) carry[i] = src[n_wide - p.fill + i];
        }
        for (int64_t r = p.record0 + (p.records > survey::RING ? p.records - survey::RING : 0); r < p.record0 + p.records; r++) {
            const float index = (float)r;
            std::fwrite(&index, sizeof(float), 1, fo);
            std::fwrite(ring.data() + (size_t)(r % survey::RING) * survey::N, sizeof(float), survey::N, fo);
        }
        fill = p.fill; blocks += p.blocks; pos += n_wide;
    }
    std::fclose(fo);
    return 0;
}
