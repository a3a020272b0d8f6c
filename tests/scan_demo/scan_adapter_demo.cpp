// scan_adapter_demo.cpp -- the C++ adapter (sdr-j-fm_amd/host/fm_processor_adapter.h) in scan mode, driven as RadioInterface drives the
// reference's fmProcessor during an automatic frequency search (radio.cpp:1115-1158): blocks before, during and after startScanning /
// stopScanning.  Prints the frames the sink received in each phase and the scan records, `found` among them (what scanresult () is emitted for).
// Used by tests/test_gpu_scan.py::test_cpp_adapter_scan.
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
struct CountSink : fmx_host::AudioSink {
    size_t frames = 0;
    int32_t putSamples(std::complex<float> *, int32_t n) override { frames += (size_t)n; return n; }
};

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s iq.f32\n", argv[0]); return 2; }
    MemDevice dev; CountSink sink;
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    dev.data.resize((size_t)bytes / sizeof(std::complex<float>));
    if (std::fread(dev.data.data(), 1, (size_t)bytes, fi) != (size_t)bytes) return 2;
    std::fclose(fi);
    fmx_host::FmProcessor p(&dev, &sink);
    if (!p.ok()) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
    p.setBandwidth("165kHz"); p.setlfcutoff(15000); p.setDeemphasis(50); p.setVolume(-6.0f);
    p.setScanThreshold(20);
    size_t frames[3] = {0, 0, 0};
    int records = 0, found = 0;
    for (int phase = 0; phase < 3; phase++) {
        if (phase == 1) p.startScanning();
        if (phase == 2) p.stopScanning();
        const size_t before = sink.frames;
        for (int b = 0; b < 8; b++) {
            if (!p.run_block()) { std::fprintf(stderr, "fmx: %s\n", p.lastError().c_str()); return 1; }
            p.poll_scan([&](const fmx_scan_result &r) { records++; if (r.found) found++; });
        }
        frames[phase] = sink.frames - before;
    }
    std::printf("frames %zu %zu %zu records %d found %d\n", frames[0], frames[1], frames[2], records, found);
    return 0;
}
