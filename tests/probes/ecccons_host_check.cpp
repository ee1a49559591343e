// Stand-alone host program: the argument checks of n2v_ecccons_* (csrc/n2v_ecccons.hip) and the tile arithmetic of the
// compaction, meant to be built with a HOST sanitizer and run on a machine without a GPU.  Every call below is refused
// before anything is launched, or has a size of 0, so no device is touched.
//
//   cd node2vec-by-ecc_amd/csrc
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I. -I../../include -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tests/probes/ecccons_host_check.cpp n2v_ecccons.hip n2v_eccsplit.hip \
//         -o /tmp/ecccons_host_check && /tmp/ecccons_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "n2v_common.h"
#include "n2v_sim.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAILED: %s (last error: %s)\n", what, n2v::err_buf()); ++failures; }
}

int main() {
    const int64_t big = (int64_t)1 << 31, tile = n2v_eccsplit_tile();
    double d[8] = {0};
    float f[8] = {0};
    int64_t i64[8] = {0};
    int32_t i32[8] = {0};
    // tile arithmetic of the compaction: ceil(n / tile) words of scratch
    expect(tile == N2V_ECCSPLIT_TILE, "tile");
    const int64_t sizes[] = {0, 1, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 5, big - 1};
    for (int64_t n : sizes) expect(n2v_eccsplit_scratch(n) == (n + tile - 1) / tile, "scratch words");
    expect(n2v_eccsplit_scratch(-3) == 0, "scratch of a negative size");
    expect(N2V_ECCCONS_CELLS / N2V_ECCCONS_MAX_BINS >= 1 && 64 * 64 <= N2V_ECCCONS_CELLS, "stripe rows");
    for (int n = 65; n <= N2V_ECCCONS_MAX_BINS; ++n) expect((N2V_ECCCONS_CELLS / n) * n <= N2V_ECCCONS_CELLS && N2V_ECCCONS_CELLS / n >= 16, "stripe fits");

    // sizes of 0 launch nothing
    expect(n2v_ecccons_check_i32(nullptr, 0, 1, 7, nullptr, nullptr) == N2V_OK, "check_i32 n = 0");
    expect(n2v_ecccons_check_i64(nullptr, 0, 0, 7, nullptr, nullptr) == N2V_OK, "check_i64 n = 0");
    expect(n2v_ecccons_profile(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 7, 0, nullptr, nullptr) == N2V_OK, "profile without users");
    expect(n2v_ecccons_features(nullptr, 0, nullptr, nullptr, 0, 0, 0, nullptr, 7, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) == N2V_OK,
           "features without rows");

    // refusals: limits, negative sizes, null pointers, bin counts
    expect(n2v_ecccons_check_i32(i32, big, 1, 7, i32, nullptr) == N2V_ERR_INVALID, "check_i32 n = 2^31");
    expect(n2v_ecccons_check_i32(i32, -1, 1, 7, i32, nullptr) == N2V_ERR_INVALID, "check_i32 n < 0");
    expect(n2v_ecccons_check_i32(nullptr, 4, 1, 7, i32, nullptr) == N2V_ERR_INVALID, "check_i32 null");
    expect(n2v_ecccons_check_i64(i64, 4, 0, 7, nullptr, nullptr) == N2V_ERR_INVALID, "check_i64 null status");
    expect(n2v_ecccons_check_ptr(i64, 0, 0, i32, nullptr) == N2V_ERR_INVALID, "check_ptr without segments");
    expect(n2v_ecccons_check_ptr(i64, 4, -1, i32, nullptr) == N2V_ERR_INVALID, "check_ptr total < 0");
    expect(n2v_ecccons_check_ptr(nullptr, 4, 4, i32, nullptr) == N2V_ERR_INVALID, "check_ptr null");
    expect(n2v_ecccons_join(d, d, i64, i64, 4, 4, i64, i64, d, d, nullptr, nullptr) == N2V_ERR_INVALID, "join null count");
    expect(n2v_ecccons_join(d, d, i64, i64, big, 4, i64, i64, d, d, i64, nullptr) == N2V_ERR_INVALID, "join n = 2^31");
    expect(n2v_ecccons_join(d, d, i64, i64, 4, -1, i64, i64, d, d, i64, nullptr) == N2V_ERR_INVALID, "join min_count < 0");
    expect(n2v_ecccons_join(d, nullptr, i64, i64, 4, 4, i64, i64, d, d, i64, nullptr) == N2V_ERR_INVALID, "join null values");
    expect(n2v_ecccons_crosstab(i32, i32, 4, 0, i64, i64, d, nullptr) == N2V_ERR_INVALID, "crosstab n = 0");
    expect(n2v_ecccons_crosstab(i32, i32, 4, N2V_ECCCONS_MAX_BINS + 1, i64, i64, d, nullptr) == N2V_ERR_INVALID, "crosstab n = 257");
    expect(n2v_ecccons_crosstab(i32, i32, -1, 7, i64, i64, d, nullptr) == N2V_ERR_INVALID, "crosstab m < 0");
    expect(n2v_ecccons_crosstab(i32, nullptr, 4, 7, i64, i64, d, nullptr) == N2V_ERR_INVALID, "crosstab null bins");
    expect(n2v_ecccons_crosstab(i32, i32, 4, 7, nullptr, i64, d, nullptr) == N2V_ERR_INVALID, "crosstab null count");
    expect(n2v_ecccons_profile(i64, i64, 2, i64, d, 4, i32, 3, 0, 0, d, nullptr) == N2V_ERR_INVALID, "profile n_bins = 0");
    expect(n2v_ecccons_profile(i64, i64, 2, i64, d, 4, i32, 3, 257, 0, d, nullptr) == N2V_ERR_INVALID, "profile n_bins = 257");
    expect(n2v_ecccons_profile(i64, i64, big, i64, d, 4, i32, 3, 7, 0, d, nullptr) == N2V_ERR_INVALID, "profile n_users = 2^31");
    expect(n2v_ecccons_profile(i64, i64, 2, i64, d, 4, i32, 0, 7, 0, d, nullptr) == N2V_ERR_INVALID, "profile without items");
    expect(n2v_ecccons_profile(i64, nullptr, 2, i64, d, 4, i32, 3, 7, 0, d, nullptr) == N2V_ERR_INVALID, "profile null perm");
    expect(n2v_ecccons_feature_rows(i64, d, 4, 3, i32, 2, i64, i64, d, nullptr, nullptr) == N2V_ERR_INVALID, "feature_rows null count");
    expect(n2v_ecccons_feature_rows(i64, d, big, 3, i32, 2, i64, i64, d, i64, nullptr) == N2V_ERR_INVALID, "feature_rows n_rows = 2^31");
    expect(n2v_ecccons_feature_rows(i64, d, 4, 3, i32, -1, i64, i64, d, i64, nullptr) == N2V_ERR_INVALID, "feature_rows n_vec < 0");
    expect(n2v_ecccons_feature_rows(nullptr, d, 4, 3, i32, 2, i64, i64, d, i64, nullptr) == N2V_ERR_INVALID, "feature_rows null item");
    expect(n2v_ecccons_features(i64, 5, i64, i64, 4, 2, 3, d, 7, i32, f, 2, 2, nullptr, d, nullptr) == N2V_ERR_INVALID, "features kept > rows");
    expect(n2v_ecccons_features(i64, 2, i64, i64, 4, 2, 3, d, 7, nullptr, f, 2, 2, nullptr, d, nullptr) == N2V_ERR_INVALID, "features vec without slots");
    expect(n2v_ecccons_features(i64, 2, i64, i64, 4, 2, 3, d, 7, i32, f, 2, 0, nullptr, d, nullptr) == N2V_ERR_INVALID, "features d = 0");
    expect(n2v_ecccons_features(i64, 2, i64, i64, 4, 2, 3, d, 7, nullptr, nullptr, 0, 0, nullptr, d, nullptr) == N2V_ERR_INVALID, "features without vec or values");
    expect(n2v_ecccons_features(i64, 2, i64, i64, 4, 2, 3, d, 300, nullptr, nullptr, 0, 0, d, d, nullptr) == N2V_ERR_INVALID, "features n_bins = 300");
    expect(std::strlen(n2v::err_buf()) > 0, "a refusal leaves a message");
    std::printf(failures ? "%d check(s) failed\n" : "ecccons host checks: all refused or empty as stated\n", failures);
    return failures != 0;
}
