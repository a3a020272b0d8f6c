// feed_adapter_demo.cpp -- the monitoring feed through the C++ adapter (sdr-j-fm_amd/host/fm_processor_adapter.h): fmx_feed_info and fmx_feed_taps without
// a device, then setFeed (1), blocks of the file, pollFeed after every block.  Writes per feed block its index (as f32), its power and its 160 samples
// to the output file, then polls once as 16 bit, and prints `blocks <n> first <b>`.  Used by tests/test_gpu_feed.py; tests/test_feed_cpu.py compiles it and
// runs the part that needs no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "fm_processor_adapter.h"

struct MemDevice : fmx_host::DeviceHandler {
    std::vector<std::complex<float>> data; size_t pos = 0;
    int32_t Samples() override { return (int32_t)(data.size() - pos); }
    int32_t getSamples(std::complex<float> *dst, int32_t n) override {
        std::memcpy(dst, data.data() + pos, sizeof(std::complex<float>) * (size_t)n); pos += (size_t)n; return n;
    }
};
struct NullSink : fmx_host::AudioSink {
    int32_t putSamples(std::complex<float> *, int32_t n) override { return n; }
};

int main(int argc, char **argv) {
    fmx_feed_info_t info{};
    if (fmx_feed_info(&info) != FMX_OK) return 4;
    float h[144]; int32_t nh = 0;
    if (fmx_feed_taps(h, 144, &nh) != FMX_OK || nh != 144) return 4;
    double sum = 0.0;
    for (int k = 0; k < nh; k++) sum += (double)h[k];
    std::printf("info rate %d block %d frames %d lookback %d delay %.1f ring %d bytes %d taps %d sum %.6f\n", info.rate_hz, info.block_samples, info.block_frames,
                info.lookback_frames, info.delay_frames, info.ring_blocks, info.bytes_per_channel, nh, sum);
    if (argc < 3) { std::fprintf(stderr, "usage: %s iq.f32 blocks.bin\n", argv[0]); return 2; }
    MemDevice dev; NullSink sink;
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    dev.data.resize((size_t)bytes / sizeof(std::complex<float>));
    if (std::fread(dev.data.data(), 1, (size_t)bytes, fi) != (size_t)bytes) return 2;
    std::fclose(fi);
    fmx_host::FmProcessor p(&dev, &sink);
    if (!p.ok()) { std::printf("ok 0 error %s\n", p.lastError().c_str()); return 3; }
    if (p.setFeed(4)) return 1;                                            // (no such mode)
    if (!p.setFeed(1)) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    size_t blocks = 0, blocks16 = 0; long long first = -1;
    while (dev.Samples() >= 2 * 16384) {
        if (!p.run_block()) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
        p.pollFeed([&](int64_t b, const float *audio, float power) {
            const float index = (float)b;
            std::fwrite(&index, sizeof(float), 1, fo); std::fwrite(&power, sizeof(float), 1, fo); std::fwrite(audio, sizeof(float), 160, fo);
            if (first < 0) first = (long long)b;
            blocks++;
        });
    }
    std::fclose(fo);
    // the last block of the file as 16 bit
    if (dev.Samples() >= 16384 && !p.run_block()) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
    int peak = 0;
    p.pollFeedS16([&](int64_t, const int16_t *audio, float) { for (int i = 0; i < 160; i++) if (std::abs((int)audio[i]) > peak) peak = std::abs((int)audio[i]); blocks16++; });
    std::printf("s16 blocks %zu peak %s\n", blocks16, peak > 0 ? "nonzero" : "zero");
    std::printf("blocks %zu first %lld\n", blocks, first);
    return 0;
}
