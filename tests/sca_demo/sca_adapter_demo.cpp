// sca_adapter_demo.cpp -- the sub-carrier decoder through the C++ adapter (sdr-j-fm_amd/host/fm_processor_adapter.h): fmx_sca_info and fmx_sca_taps
// without a device, then setScaSetup (defaults), setScaDecoder (67 000), blocks of the file, pollSca after every block.  Writes per decoder block its
// index (as f32), its level and its 240 audio samples to the output file and prints `blocks <n> first <b>`.  Used by tests/test_gpu_sca.py;
// tests/test_sca_cpu.py compiles it and runs the part that needs no device.
#include <cstdio>
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
    fmx_sca_info_t info{};
    if (fmx_sca_info(192000, &info) != FMX_OK) return 4;
    float g[192]; int32_t ng = 0;
    if (fmx_sca_taps(nullptr, 192000, 0, g, 192, &ng) != FMX_OK || ng != 192) return 4;
    double sum = 0.0;
    for (int k = 0; k < ng; k++) sum += (double)g[k];
    std::printf("info rate %d block %d fm %d lookback %d delay %.1f ring %d bytes %d taps %d sum %.6f\n", info.audio_rate_hz, info.block_audio, info.block_fm,
                info.lookback_fm, info.delay_fm, info.ring_blocks, info.bytes_per_channel, ng, sum);
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
    if (!p.setScaSetup(nullptr)) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
    if (p.setScaDecoder(92000)) return 1;                                  // (refused at 192 kS/s)
    if (!p.setScaDecoder(67000)) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    size_t blocks = 0; long long first = -1;
    while (dev.Samples() >= 16384) {
        if (!p.run_block()) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
        p.pollSca([&](int64_t b, const float *audio, float level) {
            const float index = (float)b;
            std::fwrite(&index, sizeof(float), 1, fo); std::fwrite(&level, sizeof(float), 1, fo); std::fwrite(audio, sizeof(float), 240, fo);
            if (first < 0) first = (long long)b;
            blocks++;
        });
    }
    std::fclose(fo);
    std::printf("blocks %zu first %lld\n", blocks, first);
    return 0;
}
