// spec_check.cpp -- the spectrum meter's pure functions (sdr-j-fm_amd/csrc/fmx_spec.h) and the survey's stage functions it shares (fmx_survey.h)
// compiled for the host and driven as fmx_spec.hip and stage_spectrum drive them: piece by piece, launch by launch (spec::launches), thread by thread,
// pass by pass, with one LDS image, one carry, one sum and one maximum per bin and a ring of four records.  tests/test_spec_cpu.py sets the result
// ("kernel_form") against the float64 model of tests/spec_model.py.
//
//   spec_check spectrum in.c64 out.f32 B S on_call scratch_blocks [call lengths ...]
//       in: one stream of complex f32 samples from g = 0, cut into calls of the given lengths (none: one call); the meter is switched on by call
//       `on_call` (0: from the start).  The scratch holds scratch_blocks blocks: a small number cuts a call's blocks into chunks.  out: one row of
//       1 + 2 * 4096 f32 per record delivered, written behind the call that completed it if it was still in the ring: index, mean, peak.
//   spec_check plan g0 n S B [...]
//       prints spec::piece's answer for every four numbers: b0 blocks fill fill_after append carry_src phase record0 records
//   spec_check launches streams scratch_blocks blocks carries [...]
//       prints spec::launches' visits for every four numbers, one line `j0 gn done nb write_carry` each, and a line `end`
//   spec_check rules g S B r
//       prints first_block (g, S), delivered (r, B, first_block) and record_end (r, B, S)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdr-j-fm_amd/csrc/fmx_spec.h"

using namespace fmx;

static int run_plan(int argc, char **argv) {
    for (int a = 2; a + 3 < argc; a += 4) {
        const spec::Piece p = spec::piece(std::atoll(argv[a]), std::atoll(argv[a + 1]), (int32_t)std::atoi(argv[a + 2]), (int32_t)std::atoi(argv[a + 3]));
        std::printf("%lld %lld %d %d %d %lld %d %lld %lld\n", (long long)p.b0, (long long)p.blocks, (int)p.fill, (int)p.fill_after, (int)p.append,
                    (long long)p.carry_src, (int)p.phase, (long long)p.record0, (long long)p.records);
    }
    return 0;
}

static int run_launches(int argc, char **argv) {
    for (int a = 2; a + 3 < argc; a += 4) {
        spec::launches(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), std::atoi(argv[a + 3]) != 0,
                       [](int64_t j0, int64_t gn, int64_t done, int64_t nb, bool wc) {
                           std::printf("%lld %lld %lld %lld %d\n", (long long)j0, (long long)gn, (long long)done, (long long)nb, wc ? 1 : 0);
                       });
        std::printf("end\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return run_plan(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "launches")) return run_launches(argc, argv);
    if (argc == 6 && !std::strcmp(argv[1], "rules")) {
        const int64_t g = std::atoll(argv[2]), r = std::atoll(argv[5]);
        const int32_t S = (int32_t)std::atoi(argv[3]), B = (int32_t)std::atoi(argv[4]);
        const int64_t first = spec::first_block(g, S);
        std::printf("%lld %d %lld\n", (long long)first, spec::delivered(r, B, first) ? 1 : 0, (long long)spec::record_end(r, B, S));
        return 0;
    }
    if (argc == 7 && !std::strcmp(argv[1], "fold")) {
        // spec_check fold powers.f32 out.f32 B first chunk: spec::fold over the blocks 0 .. of powers [blocks][4096], `chunk` blocks per call, sum and
        // maximum carried between the calls as fmx_spec.hip carries them -> per delivered record a row of index, mean, peak
        FILE *fp = std::fopen(argv[2], "rb");
        if (!fp) return 2;
        std::fseek(fp, 0, SEEK_END); const long pb = std::ftell(fp); std::fseek(fp, 0, SEEK_SET);
        std::vector<float> pw((size_t)pb / sizeof(float));
        if (std::fread(pw.data(), sizeof(float), pw.size(), fp) != pw.size()) return 2;
        std::fclose(fp);
        const int B = std::atoi(argv[4]);
        const int64_t first = std::atoll(argv[5]), chunk = std::atoll(argv[6]), nb = (int64_t)(pw.size() / spec::N);
        if (B < 1 || chunk < 1) return 2;
        std::vector<float> window(spec::N), acc((size_t)2 * spec::N, 0.f), ring((size_t)spec::RING * 2 * spec::N, 0.f);
        survey::make_window(window.data());
        const float c = survey::record_scale(window.data(), B), c1 = survey::record_scale(window.data(), 1);
        FILE *fo = std::fopen(argv[3], "wb");
        if (!fo) return 2;
        for (int64_t b = 0; b < nb; b += chunk) {
            const int64_t m = std::min(chunk, nb - b);
            for (int i = 0; i < spec::N; i++)
                spec::fold(acc[i], acc[spec::N + i], pw.data() + (size_t)b * spec::N + i, spec::N, b, m, first, (int)(b % B), B, c, c1, ring.data() + i,
                           ring.data() + spec::N + i);
            for (int64_t r = b / B; r < (b + m) / B; r++) {
                if (!spec::delivered(r, B, first) || r < (b + m) / B - spec::RING) continue;
                const float index = (float)r;
                std::fwrite(&index, sizeof(float), 1, fo);
                std::fwrite(ring.data() + (size_t)(r % spec::RING) * 2 * spec::N, sizeof(float), (size_t)2 * spec::N, fo);
            }
        }
        std::fclose(fo);
        return 0;
    }
    if (argc < 8 || std::strcmp(argv[1], "spectrum")) { std::fprintf(stderr, "usage: see the head of spec_check.cpp\n"); return 2; }
    FILE *fi = std::fopen(argv[2], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); const long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    std::vector<float2> in((size_t)bytes / sizeof(float2));
    if (std::fread(in.data(), sizeof(float2), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);
    const int B = std::atoi(argv[4]), S = std::atoi(argv[5]), on_call = std::atoi(argv[6]);
    const int64_t scratch = std::atoll(argv[7]);
    if (B < 1 || B > spec::MAX_B || S < 1 || S > spec::MAX_S || scratch < 1) return 2;
    std::vector<int64_t> calls;
    int64_t sum = 0;
    for (int a = 8; a < argc; a++) { calls.push_back(std::atoll(argv[a])); sum += calls.back(); }
    if (calls.empty()) calls.push_back((int64_t)in.size());
    else if (sum != (int64_t)in.size()) return 2;

    std::vector<float> window(spec::N);
    std::vector<float2> W(spec::N), carry(spec::N), lds(survey::LDS_N), regs((size_t)spec::NT * spec::PER);
    survey::make_window(window.data());
    survey::make_twiddles(W.data());
    const float c = survey::record_scale(window.data(), B), c1 = survey::record_scale(window.data(), 1);
    std::vector<float> acc((size_t)2 * spec::N, 0.f), ring((size_t)spec::RING * 2 * spec::N, 0.f), power((size_t)scratch * spec::N);
    FILE *fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    int64_t g0 = 0, on_from = -1;
    int k = 0;
    for (const int64_t n : calls) {
        const float2 *src = in.data() + g0;
        if (k++ >= on_call) {
            if (on_from < 0) on_from = g0;
            const int64_t first = spec::first_block(on_from, S);
            const spec::Piece p = spec::piece(g0, n, S, B);
            spec::launches(1, scratch, p.blocks, p.fill_after > 0, [&](int64_t, int64_t, int64_t done, int64_t nb, bool write_carry) {
                for (int64_t j = 0; j < nb; j++) {                             // spec_block_kernel, workgroup j of the chunk
                    const int64_t b = p.b0 + done + j;
                    for (int t = 0; t < spec::NT; t++) {
                        float2 x[spec::PER];
                        for (int n2 = 0; n2 < spec::PER; n2++) {
                            const int i = t + 256 * n2;
                            const int64_t q = spec::source_index(b, i, g0, S);
                            if (q >= n) std::abort();                          // (the block completes in the piece)
                            const float2 v = q < 0 ? carry[(size_t)i] : src[q];
                            x[n2] = make_float2(v.x * window[i], v.y * window[i]);
                        }
                        survey::pass1(t, x, W.data(), lds.data());
                    }
                    for (int t = 0; t < spec::NT; t++) survey::pass2_load(t, lds.data(), &regs[(size_t)t * spec::PER]);
                    for (int t = 0; t < spec::NT; t++) survey::pass2_store(t, &regs[(size_t)t * spec::PER], W.data(), lds.data());
                    for (int t = 0; t < spec::NT; t++) {
                        float pw[spec::PER];
                        survey::pass3(t, lds.data(), W.data(), pw);
                        for (int cc = 0; cc < spec::PER; cc++) power[(size_t)j * spec::N + t + 256 * cc] = pw[cc];
                    }
                }
                for (int i = 0; i < spec::N; i++) {                            // spec_fold_kernel, thread i
                    if (nb > 0)
                        spec::fold(acc[i], acc[spec::N + i], power.data() + i, spec::N, p.b0 + done, nb, first, (int)((p.b0 + done) % B), B, c, c1,
                                   ring.data() + i, ring.data() + spec::N + i);
                    if (!write_carry) continue;
                    if (p.append) { if (i < n) carry[(size_t)(p.fill + i)] = src[i]; }
                    else if (i < p.fill_after) carry[i] = src[p.carry_src + i];
                }
            });
            const int64_t r_end = p.record0 + p.records;
            for (int64_t r = std::max(p.record0, r_end - spec::RING); r < r_end; r++) {
                if (!spec::delivered(r, B, first)) continue;
                const float index = (float)r;
                std::fwrite(&index, sizeof(float), 1, fo);
                std::fwrite(ring.data() + (size_t)(r % spec::RING) * 2 * spec::N, sizeof(float), (size_t)2 * spec::N, fo);
            }
        }
        g0 += n;
    }
    std::fclose(fo);
    return 0;
}
