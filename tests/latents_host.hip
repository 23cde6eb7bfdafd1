// Stand-alone host program for tests/test_latents.py: runs the work items of csrc/latents.hip (latent_plan, latent_item -- host and device
// functions) over host memory, between guard zones, and writes z and bits to files.  No device is touched.
//   latents_host DIRS OUT n K R zdim first_agent seed kind scramble antithetic center truncate
// exit: 0 written; 2 the call is refused (reason on stderr); 3 bad DIRS; 4 a guard word was written; 5 an element was left unwritten
#include "../sttode_amd/csrc/latents.hip"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

void stt_set_error(const char*) {}
int stt_refuse(const char* who, const char* why) {
    fprintf(stderr, "%s: %s\n", who, why);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 14) return 1;
    const int n = atoi(argv[3]), K = atoi(argv[4]), R = atoi(argv[5]), zdim = atoi(argv[6]);
    const long long first_agent = atoll(argv[7]);
    const unsigned long long seed = strtoull(argv[8], nullptr, 10);
    const int kind = atoi(argv[9]), scramble = atoi(argv[10]), antithetic = atoi(argv[11]), center = atoi(argv[12]);
    const float truncate = (float)atof(argv[13]);
    std::vector<unsigned> dirs((size_t)zdim * 30);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(dirs.data(), 4, dirs.size(), f) != dirs.size()) return 3;
    fclose(f);
    const size_t tot = (size_t)R * n * K * zdim, G = 64;                // 64 guard words on either side, 16-byte aligned payload
    const float fill = 12345.0f;
    std::vector<float> zb(tot + 2 * G + 4, fill);
    std::vector<int> bb(tot + 2 * G + 4, -99);
    float* z = zb.data() + G;
    int* bits = bb.data() + G;
    while ((uintptr_t)z & 15) ++z;
    while ((uintptr_t)bits & 15) ++bits;
    LatentArgs A;
    if (const char* why = latent_plan(A, z, bits, dirs.data(), n, K, R, zdim, first_agent, seed, kind, scramble, antithetic, center, truncate)) {
        fprintf(stderr, "refused: %s\n", why);
        return 2;
    }
    const bool vec = latent_vec(A);
    for (long long it = 0; it < A.total; ++it) {
        if (vec) latent_item<true>(A, it);
        else latent_item<false>(A, it);
    }
    for (float* p = zb.data(); p < zb.data() + zb.size(); ++p)
        if ((p < z || p >= z + tot) && *p != fill) return 4;
    for (int* p = bb.data(); p < bb.data() + bb.size(); ++p)
        if ((p < bits || p >= bits + tot) && *p != -99) return 4;
    for (size_t i = 0; i < tot; ++i)
        if (z[i] == fill) return 5;                                      // (|z| <= 6.34; a bits word left at -99 shows against the restatement)
    const std::string out = argv[2];
    f = fopen((out + ".z").c_str(), "wb");
    fwrite(z, 4, tot, f);
    fclose(f);
    f = fopen((out + ".bits").c_str(), "wb");
    fwrite(bits, 4, tot, f);
    fclose(f);
    printf("%d %lld\n", (int)vec, A.total);
    return 0;
}
