// Stand-alone host run of astrild_amd/csrc/ray_step.h (built with -fsanitize=address,undefined,float-cast-overflow by
// tests/test_ray_step_host.py): one plane's step over every ray of a case file, then the emit of one source, written
// out as raw doubles for the byte comparison with tests/ray_trace_oracle.py.  Every buffer is a std::vector of exactly
// the size the contract names, so a read or a write outside psi, the state or the maps is reported.
//
//   ray_step_test CASE OUT
//   CASE: int64 m, npix, born; double h, chi_prev, chi_k, chi_s; psi (m x m doubles); state (12 x npix x npix doubles)
//   OUT : the state after the step (12 x npix x npix), then the six maps (6 x npix x npix)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ray_step.h"

static bool read_all(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s CASE OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    int64_t dims[3];
    double par[4];
    if (!read_all(in, dims, sizeof dims) || !read_all(in, par, sizeof par)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int64_t m = dims[0], npix = dims[1], born = dims[2];
    const double h = par[0], chi_prev = par[1], chi_k = par[2], chi_s = par[3];
    if (m < 1 || m > 4096 || npix < 1 || npix > m || (born != 0 && born != 1)) { std::fprintf(stderr, "bad header\n"); return 2; }
    const size_t plane = (size_t)npix * (size_t)npix;
    std::vector<double> psi((size_t)m * (size_t)m), state(ast_ray::STATE_PLANES * plane), maps(ast_ray::EMIT_PLANES * plane);
    if (!read_all(in, psi.data(), psi.size() * sizeof(double)) || !read_all(in, state.data(), state.size() * sizeof(double)) ||
        std::fgetc(in) != EOF) {
        std::fprintf(stderr, "case file does not hold exactly psi and the state\n");
        return 2;
    }
    std::fclose(in);
    const double dchi = chi_k - chi_prev;                        // formed by the caller, as ast_ray_step does
    for (int i = 0; i < (int)npix; ++i)
        for (int j = 0; j < (int)npix; ++j) {
            if (born) ast_ray::step_ray<true>(psi.data(), state.data(), (int)m, (int)npix, i, j, h, chi_prev, dchi, chi_k);
            else ast_ray::step_ray<false>(psi.data(), state.data(), (int)m, (int)npix, i, j, h, chi_prev, dchi, chi_k);
        }
    for (size_t e = 0; e < plane; ++e)
        ast_ray::emit_ray(state.data(), plane, e, chi_k, chi_s - chi_k, chi_s, maps.data(), plane);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    const bool ok = std::fwrite(state.data(), sizeof(double), state.size(), out) == state.size() &&
                    std::fwrite(maps.data(), sizeof(double), maps.size(), out) == maps.size();
    if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
    std::printf("ray_step: m %lld npix %lld born %lld: %zu rays stepped and emitted\n", (long long)m, (long long)npix,
                (long long)born, plane);
    return 0;
}
