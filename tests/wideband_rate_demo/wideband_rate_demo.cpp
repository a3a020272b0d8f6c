// wideband_rate_demo.cpp -- the C++ wrapper of stage W (sdr-j-fm_amd/host/wideband_adapter.h) with a rate object, driven as the thread of a
// fixed-rate receiver would: one wide stream from a raw F32 file, processHost in two calls with a setOffset between them, each call's count
// asked for with outputsFor, the narrow streams written to a file ([outputs][count of the whole stream] complex f32).  Prints
// `taps <n> <L> <M>` (the prototype needs no device), then `ok 1 ...`, or `ok 0 error <text>` and exit code 3 where the object could not be
// created (no device).  Used by tests/test_gpu_wideband_rate.py::test_cpp_adapter.
#include <cstdio>
#include <cstdlib>
#include "wideband_adapter.h"

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s wide.f32 narrow.f32 rate_hz n_first retuned_output retuned_hz offset_hz...\n", argv[0]);
        return 2;
    }
    const int32_t rate = (int32_t)std::atoi(argv[3]);
    const int64_t n_first = std::atoll(argv[4]);
    const int32_t retuned = (int32_t)std::atoi(argv[5]), retuned_hz = (int32_t)std::atoi(argv[6]);
    std::vector<int32_t> offs, sof;
    for (int a = 7; a < argc; a++) { offs.push_back((int32_t)std::atoi(argv[a])); sof.push_back(0); }
    int32_t L = 0, M = 0;
    const size_t n_taps = fmx_host::Wideband::rateTaps(rate, &L, &M).size();
    std::printf("taps %zu %d %d\n", n_taps, (int)L, (int)M);
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); const long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    std::vector<float> wide((size_t)bytes / sizeof(float));
    if (std::fread(wide.data(), 1, (size_t)bytes, fi) != (size_t)bytes) return 2;
    std::fclose(fi);
    const int64_t n = (int64_t)(wide.size() / 2);
    if (n_taps == 0 || n_first < 0 || n_first > n) return 2;
    fmx_host::Wideband w(fmx_host::Wideband::Rate{rate}, 1, sof, offs, (int32_t)n);
    if (!w.ok()) { std::printf("ok 0 error %s\n", w.lastError().c_str()); return 3; }
    std::printf("ok 1 factor %d outputs %d\n", (int)w.factor(), (int)w.outputs());
    const int64_t n_out = n * L / M;                                    // the whole stream's count: floor (n L / M)
    std::vector<float> narrow((size_t)w.outputs() * (size_t)n_out * 2);
    const int64_t want_first = w.outputsFor(n_first);
    int64_t got = 0;
    if (!w.processHost(wide.data(), FMX_IQ_F32, 2048.0f, n, n_first, narrow.data(), n_out, &got) || got != want_first) {
        std::fprintf(stderr, "fmx: %s\n", w.lastError().c_str()); return 1;
    }
    if (!w.setOffset(retuned, retuned_hz)) { std::fprintf(stderr, "fmx: %s\n", w.lastError().c_str()); return 1; }
    const int64_t want_rest = w.outputsFor(n - n_first);
    if (want_first + want_rest != n_out) { std::fprintf(stderr, "counts %lld + %lld != %lld\n", (long long)want_first, (long long)want_rest, (long long)n_out); return 1; }
    if (!w.processHost(wide.data() + 2 * n_first, FMX_IQ_F32, 2048.0f, n - n_first, n - n_first, narrow.data() + 2 * got, n_out, &got) ||
        got != want_rest) {
        std::fprintf(stderr, "fmx: %s\n", w.lastError().c_str()); return 1;
    }
    std::printf("counts %lld %lld\n", (long long)want_first, (long long)want_rest);
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(narrow.data(), sizeof(float), narrow.size(), fo) != narrow.size()) return 2;
    std::fclose(fo);
    return 0;
}
