// mpx_adapter_demo.cpp -- the multiplex spectrum meter through the C++ adapter (sdr-j-fm_amd/host/fm_processor_adapter.h): setMpxSpectrumGrid (2, 1),
// setMpxSpectrumMeter, blocks of the file, pollMpxSpectrum after every block, mpxFigures over the last record.  Writes per record its index (as f32), mean
// and peak (2048 f32 each) to the output file and prints `records <n> total <Hz> pilot <Hz> at <Hz>` in the demodulator's own units.  Used by
// tests/test_gpu_mpx_spectrum.py; tests/test_mpx_cpu.py compiles it and runs the part that needs no device.
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
    static_assert(sizeof(fmx_mpx_record) == 24, "fmx_mpx_record is 24 bytes");
    fmx_mpx_find cfg{};
    cfg.struct_size = (int32_t)sizeof(cfg); cfg.rate_hz = 192000; cfg.hz_per_unit = 1.0; cfg.dc_guard_hz = 30; cfg.line_half_hz = 1;
    fmx_mpx_figs f0;
    std::vector<float> flat(2048, 1.0f);
    if (fmx_host::FmProcessor::mpxFigures(&cfg, flat.data(), nullptr, &f0)) return 4;          // (line_half_hz = 1 is refused, and needs no device)
    cfg.line_half_hz = 250;
    if (!fmx_host::FmProcessor::mpxFigures(&cfg, flat.data(), nullptr, &f0)) return 4;
    std::printf("figures 1 pilot_freq %.6f\n", f0.pilot_freq_hz);
    if (argc < 3) { std::fprintf(stderr, "usage: %s iq.f32 records.bin\n", argv[0]); return 2; }
    MemDevice dev; NullSink sink;
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    dev.data.resize((size_t)bytes / sizeof(std::complex<float>));
    if (std::fread(dev.data.data(), 1, (size_t)bytes, fi) != (size_t)bytes) return 2;
    std::fclose(fi);
    fmx_host::FmProcessor p(&dev, &sink);
    if (!p.ok()) { std::printf("ok 0 error %s\n", p.lastError().c_str()); return 3; }
    if (!p.setMpxSpectrumGrid(2, 1)) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
    p.setMpxSpectrumMeter(true);
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    size_t records = 0;
    std::vector<float> last_mean(2048), last_peak(2048);
    while (dev.Samples() >= 16384) {
        if (!p.run_block()) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
        p.pollMpxSpectrum([&](const fmx_mpx_record &r, const float *mean, const float *peak) {
            const float index = (float)r.index;
            std::fwrite(&index, sizeof(float), 1, fo); std::fwrite(mean, sizeof(float), 2048, fo); std::fwrite(peak, sizeof(float), 2048, fo);
            std::memcpy(last_mean.data(), mean, sizeof(float) * 2048); std::memcpy(last_peak.data(), peak, sizeof(float) * 2048);
            records++;
        });
    }
    std::fclose(fo);
    fmx_mpx_figs f{};
    if (records && !fmx_host::FmProcessor::mpxFigures(&cfg, last_mean.data(), last_peak.data(), &f)) return 1;
    std::printf("records %zu total %.17g pilot %.17g at %.17g\n", records, f.total_hz, f.pilot_hz, f.pilot_freq_hz);
    return 0;
}
