// feed_check.cpp -- the monitoring feed's pure functions (sdr-j-fm_amd/csrc/fmx_feed.h) compiled for the host and driven as stage_feed and fmx_feed.hip
// drive them: piece by piece, one carry of v, the span of every completed block staged from carry and frames, the per-sample functions in the kernel's
// order.  tests/test_feed_cpu.py sets the result (the "host form") against the float64 model and the numpy-f32 restatement of tests/feed_model.py.
//
//   feed_check blocks in.f32 out.f32 mode M_start on_call [piece lengths ...]
//       in: one channel's PCM as interleaved (L, R) f32 from frame M_start on (a multiple of 480), cut into pieces of the given lengths in frames (none:
//       one piece); the feed is switched on in `mode` by piece `on_call` (0: from the start).  out: one row of 2 + 160 f32 per delivered block:
//       b - M_start / 480, power, audio.
//   feed_check piece M0 frames on_from [...]
//       prints for every three numbers: first b0 blocks carry_from0 carry_len0 carry_from1 carry_len1 from_carry row_src formed_from ring_slot (b0)
//   feed_check s16 in.f32 out.s16
//       feed::to_s16 of every value
//   feed_check taps out.f32
//       feed::design ()
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdr-j-fm_amd/csrc/fmx_feed.h"

using namespace fmx;

static bool read_f32(const char *path, std::vector<float> &v) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END); const long bytes = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.assign((size_t)bytes / sizeof(float), 0.f);
    const bool ok = std::fread(v.data(), sizeof(float), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "piece")) {
        for (int a = 2; a + 2 < argc; a += 3) {
            const int64_t M0 = std::atoll(argv[a]), frames = std::atoll(argv[a + 1]), on = std::atoll(argv[a + 2]);
            const feed::Piece p = feed::piece(M0, frames, on);
            std::printf("%lld %lld %lld %lld %d %lld %d %d %lld %lld %d\n", (long long)feed::first_block(on), (long long)p.b0, (long long)p.blocks,
                        (long long)p.carry_from0, (int)p.carry_len0, (long long)p.carry_from1, (int)p.carry_len1, (int)p.from_carry, (long long)p.row_src,
                        (long long)feed::formed_from(M0, frames), feed::ring_slot(p.b0));
        }
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "s16")) {
        std::vector<float> in;
        if (!read_f32(argv[2], in)) return 2;
        std::vector<int16_t> out(in.size());
        for (size_t i = 0; i < in.size(); i++) out[i] = feed::to_s16(in[i]);
        FILE *fo = std::fopen(argv[3], "wb");
        if (!fo) return 2;
        std::fwrite(out.data(), sizeof(int16_t), out.size(), fo);
        std::fclose(fo);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "taps")) {
        const std::vector<float> h = feed::design();
        FILE *fo = std::fopen(argv[2], "wb");
        if (!fo) return 2;
        std::fwrite(h.data(), sizeof(float), h.size(), fo);
        std::fclose(fo);
        return 0;
    }
    if (argc < 7 || std::strcmp(argv[1], "blocks")) { std::fprintf(stderr, "usage: see the head of feed_check.cpp\n"); return 2; }
    std::vector<float> in;
    if (!read_f32(argv[2], in) || in.size() % 2) return 2;
    const int64_t n_in = (int64_t)in.size() / 2;
    const float2 *pcm = reinterpret_cast<const float2 *>(in.data());
    const int mode = std::atoi(argv[4]);
    const int64_t M_start = std::atoll(argv[5]);
    const int on_call = std::atoi(argv[6]);
    if (M_start % feed::BLOCK_FRAMES || mode < 1 || mode > 3) return 2;
    std::vector<int64_t> calls;
    int64_t sum = 0;
    for (int a = 7; a < argc; a++) { calls.push_back(std::atoll(argv[a])); sum += calls.back(); }
    if (calls.empty()) calls.push_back(n_in);
    else if (sum != n_in) return 2;

    const std::vector<float> taps = feed::design();
    alignas(16) float h_aligned[feed::NTAPS];                                                   // (feed::y_of reads the taps four per 16-byte load)
    std::memcpy(h_aligned, taps.data(), sizeof(h_aligned));
    std::vector<float> carry(feed::CARRY_STRIDE, 0.f), next(feed::CARRY_STRIDE, 0.f), span(feed::SPAN), row_out(2 + feed::BLOCK, 0.f);
    FILE *fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    int64_t M0 = M_start, on_from = -1;
    int k = 0;
    for (const int64_t frames : calls) {
        const float2 *row = pcm + (M0 - M_start);                                               // (a piece sees its own frames only)
        if (k++ >= on_call) {
            if (on_from < 0) on_from = M0;
            const feed::Piece p = feed::piece(M0, frames, on_from);
            const int64_t lo = feed::formed_from(M0, frames);
            for (int64_t b = p.b0 > lo ? p.b0 : lo; b < p.b0 + p.blocks; b++) {                 // feed_block_kernel, one workgroup each
                for (int i = 0; i < feed::SPAN; i++) {
                    const int64_t m = feed::block_from(b) + i;
                    if (m < M0 ? (m < p.carry_from0 || m - p.carry_from0 >= p.carry_len0) : (m - M0 >= frames)) std::abort();      // (the bounds the kernel relies on)
                    span[(size_t)i] = feed::span_value(b, i, M0, p.carry_from0, carry.data(), row, mode);
                }
                feed::block_host(span.data(), h_aligned, row_out.data() + 2, &row_out[1]);
                row_out[0] = (float)(b - M_start / feed::BLOCK_FRAMES);
                std::fwrite(row_out.data(), sizeof(float), row_out.size(), fo);
            }
            if (p.carry_len1 > feed::CARRY_MAX) std::abort();
            for (int i = 0; i < p.carry_len1; i++) {                                            // feed_carry_kernel: every read, then every write
                if (i < p.from_carry ? (p.carry_from1 - p.carry_from0 + i >= p.carry_len0) : (p.row_src + (i - p.from_carry) >= frames)) std::abort();
                next[(size_t)i] = feed::carry_value(p, i, carry.data(), row, mode);
            }
            for (int i = 0; i < p.carry_len1; i++) carry[(size_t)i] = next[(size_t)i];
        }
        M0 += frames;
    }
    std::fclose(fo);
    return 0;
}
