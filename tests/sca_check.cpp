// sca_check.cpp -- the sub-carrier decoder's pure functions (sdr-j-fm_amd/csrc/fmx_sca.h) compiled for the host and driven as stage_sca and fmx_sca.hip
// drive them: piece by piece, one carry, the span of every completed block staged from carry and row, the per-sample functions in the kernel's order.
// tests/test_sca_cpu.py sets the result (the "host form") against the float64 model of tests/sca_model.py.
//
//   sca_check blocks in.f32 out.f32 centre_hz J_start on_call defect [piece lengths ...]
//       in: one channel's demodulator output as f32 from fm sample J_start on (a multiple of 1920), cut into pieces of the given lengths (none: one
//       piece); the decoder (default setup, 192 kS/s) is switched on by piece `on_call` (0: from the start).  out: one row of 2 + 240 f32 per delivered
//       block: b - J_start / 1920, level, audio.
//       defect 0: none.  Seeded into THIS DRIVER's use of the header, for the detector's test: 1: a stale carry sample -- the carry write skips position
//       300; 2: the row is read one sample late in the second piece; 3: a block left out -- the fourth delivered block is not formed, its row repeats the
//       third's
//   sca_check piece J0 nj on_from [...]
//       prints sca::piece's answer for every three numbers: first b0 blocks carry_from0 carry_len0 carry_from1 carry_len1 from_carry row_src
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdr-j-fm_amd/csrc/fmx_sca.h"

using namespace fmx;

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "piece")) {
        for (int a = 2; a + 2 < argc; a += 3) {
            const int64_t J0 = std::atoll(argv[a]), nj = std::atoll(argv[a + 1]), on = std::atoll(argv[a + 2]);
            const sca::Piece p = sca::piece(J0, nj, on);
            std::printf("%lld %lld %lld %lld %d %lld %d %d %lld\n", (long long)sca::first_block(on), (long long)p.b0, (long long)p.blocks, (long long)p.carry_from0,
                        (int)p.carry_len0, (long long)p.carry_from1, (int)p.carry_len1, (int)p.from_carry, (long long)p.row_src);
        }
        return 0;
    }
    if (argc < 8 || std::strcmp(argv[1], "blocks")) { std::fprintf(stderr, "usage: see the head of sca_check.cpp\n"); return 2; }
    FILE *fi = std::fopen(argv[2], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); const long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    std::vector<float> in((size_t)bytes / sizeof(float) + 1, 0.f);          // (one more: defect 2 reads one sample late)
    if (std::fread(in.data(), sizeof(float), in.size() - 1, fi) != in.size() - 1) return 2;
    std::fclose(fi);
    const int64_t n_in = (int64_t)in.size() - 1;
    const int32_t centre = std::atoi(argv[4]), R = 192000;
    const int64_t J_start = std::atoll(argv[5]);
    const int on_call = std::atoi(argv[6]), defect = std::atoi(argv[7]);
    if (J_start % sca::BLOCK_FM) return 2;
    std::vector<int64_t> calls;
    int64_t sum = 0;
    for (int a = 8; a < argc; a++) { calls.push_back(std::atoll(argv[a])); sum += calls.back(); }
    if (calls.empty()) calls.push_back(n_in);
    else if (sum != n_in) return 2;

    const fmx_sca_config cfg = sca::default_config();
    if (sca::config_error(&cfg, R) || sca::centre_error(centre, cfg.half_band_hz, R)) return 2;
    const std::vector<float> g = sca::design_band(cfg, R), a = sca::design_audio(cfg, R);
    const std::vector<float2> c = sca::mixed_taps(g, centre, R);
    const float2 rot = sca::rotation(centre, R);
    const float scale = sca::u_scale(cfg, R);
    std::vector<float> carry(sca::CARRY_STRIDE, 0.f), next(sca::CARRY_STRIDE, 0.f), span(sca::SPAN), row_out(2 + sca::BLOCK_AUDIO, 0.f);
    FILE *fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    int64_t J0 = J_start, on_from = -1, delivered = 0;
    int k = 0;
    for (const int64_t nj : calls) {
        const float *row = in.data() + (J0 - J_start) + ((defect == 2 && k == 1) ? 1 : 0);      // (the row of a piece holds that piece's fm samples only)
        if (k++ >= on_call) {
            if (on_from < 0) on_from = J0;
            const sca::Piece p = sca::piece(J0, nj, on_from);
            for (int64_t b = p.b0; b < p.b0 + p.blocks; b++) {                                  // sca_block_kernel, one workgroup each
                if (!(defect == 3 && delivered == 3)) {
                    for (int i = 0; i < sca::SPAN; i++) {
                        const int64_t j = sca::block_from(b) + i;
                        if (j < J0 ? (j < p.carry_from0 || j - p.carry_from0 >= p.carry_len0) : (j - J0 >= nj)) std::abort();      // (the bounds the kernel relies on)
                        span[(size_t)i] = sca::span_sample(b, i, J0, p.carry_from0, carry.data(), row);
                    }
                    sca::block_host(span.data(), c.data(), a.data(), rot, scale, row_out.data() + 2, &row_out[1]);
                }
                row_out[0] = (float)(b - J_start / sca::BLOCK_FM);
                std::fwrite(row_out.data(), sizeof(float), row_out.size(), fo);
                delivered++;
            }
            if (p.carry_len1 > sca::CARRY_MAX) std::abort();
            for (int i = 0; i < p.carry_len1; i++) {                                            // sca_carry_kernel: every read, then every write
                if (i < p.from_carry ? (p.carry_from1 - p.carry_from0 + i >= p.carry_len0) : (p.row_src + (i - p.from_carry) >= nj)) std::abort();
                next[(size_t)i] = sca::carry_sample(p, i, carry.data(), row);
            }
            for (int i = 0; i < p.carry_len1; i++) if (!(defect == 1 && i == 300)) carry[(size_t)i] = next[(size_t)i];
        }
        J0 += nj;
    }
    std::fclose(fo);
    return 0;
}
