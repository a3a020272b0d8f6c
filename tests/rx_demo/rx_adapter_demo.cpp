// rx_adapter_demo.cpp -- the reception meter through the C++ adapter (sdr-j-fm_amd/host/fm_processor_adapter.h): setReceptionMeter, blocks of the file,
// pollReception after every block, receptionQuality over what the polls handed out.  Writes the fmx_rx_record of every window to the output file and prints
// `records <n> level <dB> cnr <dB> depth <d> offset <Hz>`.  Used by tests/test_gpu_rx_meter.py::test_mirrors; tests/test_rx_cpu.py compiles it.
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
    static_assert(sizeof(fmx_rx_record) == 40, "fmx_rx_record is 40 bytes");
    fmx_rx_quality q0;
    if (fmx_host::FmProcessor::receptionQuality(nullptr, 0, &q0)) return 4;      // (no records: refused, and needs no device)
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
    p.setBandwidth("165kHz");
    p.setReceptionMeter(true);
    std::vector<fmx_rx_record> recs;
    while (dev.Samples() >= 16384) {
        if (!p.run_block()) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
        p.pollReception([&](const fmx_rx_record &r) { recs.push_back(r); });
    }
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    std::fwrite(recs.data(), sizeof(fmx_rx_record), recs.size(), fo);
    std::fclose(fo);
    fmx_rx_quality q{};
    if (!recs.empty() && !fmx_host::FmProcessor::receptionQuality(recs.data(), (int32_t)recs.size(), &q)) return 1;
    std::printf("records %zu level %.17g cnr %.17g depth %.17g offset %.17g\n", recs.size(), q.level_dbfs, q.cnr_db, q.am_depth, q.offset_hz);
    return 0;
}
