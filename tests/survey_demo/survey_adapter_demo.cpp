// survey_adapter_demo.cpp -- the band survey through the C++ wrapper of stage W (sdr-j-fm_amd/host/wideband_adapter.h), as a receiver that
// starts cold would use it: one wide stream from a raw F32 file, survey (B), processHost in two calls, readSurvey, stations () of every
// record.  Writes, per record: the fmx_survey_record, its 4096 powers, the number of stations (int32), the floor (f32) and the
// fmx_survey_station of each.  Prints `finder <n>` first (stations () needs no device: an all-ones record has no station), then `ok 1`, or
// `ok 0 error <text>` and exit code 3 where the object could not be created (no device).
// Used by tests/test_gpu_survey.py::test_cpp_adapter and tests/test_survey_cpu.py.
#include <cstdio>
#include <cstdlib>
#include "wideband_adapter.h"

int main(int argc, char **argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s wide.f32 out.bin factor blocks_per_record n_first threshold_db\n", argv[0]);
        return 2;
    }
    const int32_t K = (int32_t)std::atoi(argv[3]), B = (int32_t)std::atoi(argv[4]);
    const int64_t n_first = std::atoll(argv[5]);
    const float threshold = (float)std::atof(argv[6]);
    const std::vector<float> ones(4096, 1.0f);
    std::printf("finder %zu\n", fmx_host::Wideband::stations(ones.data(), 4).size());
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    std::fseek(fi, 0, SEEK_END); const long bytes = std::ftell(fi); std::fseek(fi, 0, SEEK_SET);
    std::vector<float> wide((size_t)bytes / sizeof(float));
    if (std::fread(wide.data(), 1, (size_t)bytes, fi) != (size_t)bytes) return 2;
    std::fclose(fi);
    const int64_t n = (int64_t)(wide.size() / 2);
    if (K < 1 || n % K != 0 || n_first < 0 || n_first > n || n_first % K != 0) return 2;
    fmx_host::Wideband w(K, 1, {0}, {0}, (int32_t)n);
    if (!w.ok()) { std::printf("ok 0 error %s\n", w.lastError().c_str()); return 3; }
    std::printf("ok 1 factor %d\n", (int)w.factor());
    std::vector<float> narrow((size_t)(n / K) * 2);
    if (!w.survey(B) || !w.processHost(wide.data(), FMX_IQ_F32, 2048.0f, n, n_first, narrow.data(), n / K) ||
        !w.processHost(wide.data() + 2 * n_first, FMX_IQ_F32, 2048.0f, n - n_first, n - n_first, narrow.data(), n / K)) {
        std::fprintf(stderr, "fmx: %s\n", w.lastError().c_str()); return 1;
    }
    std::vector<fmx_survey_record> recs;
    std::vector<float> power;
    if (!w.readSurvey(0, recs, power)) { std::fprintf(stderr, "fmx: %s\n", w.lastError().c_str()); return 1; }
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    for (size_t r = 0; r < recs.size(); r++) {
        float floor_db = 0.0f;
        const std::vector<fmx_survey_station> st = fmx_host::Wideband::stations(power.data() + 4096 * r, K, 100000, 0, threshold, 0, &floor_db);
        const int32_t ns = (int32_t)st.size();
        std::fwrite(&recs[r], sizeof(fmx_survey_record), 1, fo);
        std::fwrite(power.data() + 4096 * r, sizeof(float), 4096, fo);
        std::fwrite(&ns, sizeof(ns), 1, fo);
        std::fwrite(&floor_db, sizeof(floor_db), 1, fo);
        if (ns) std::fwrite(st.data(), sizeof(fmx_survey_station), st.size(), fo);
    }
    std::fclose(fo);
    std::printf("records %zu\n", recs.size());
    return 0;
}
