// maxsim_rule_check.cpp -- stand-alone check of semcode_amd/csrc/maxsim_rule.h (the late-interaction score of one pair) on the CPU, meant
// to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Isemcode_amd/csrc scripts/maxsim_rule_check.cpp -o maxsim_rule_check
// It calls the rule the way sc_diag_maxsim_host (sc_encoder_diag.cpp) does -- heap arrays of exactly nq * W, nd * W and nd entries, so that
// an index one past either end is an error -- over edge inputs (ties, signed zeros, negative-only documents, keep masks, nd around the tile
// of 16) and random vectors, against a plain restatement.  Exit status 0 and "ok" when every case gives the expected bits.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "maxsim_rule.h"

static int failures = 0;
static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}
static void expect(const char* what, float got, float want) {
    if (bits(got) == bits(want)) return;
    ++failures;
    std::printf("FAIL %s: got %a (%08x), want %a (%08x)\n", what, got, bits(got), want, bits(want));
}

// the definition again, written without the header: the chain with explicit indices, the maximum by comparing floats and signs
static float plain(const std::vector<float>& Q, int nq, const std::vector<float>& D, int nd, const std::vector<unsigned char>* keep, int W) {
    float acc = 0.0f;
    for (int t = 0; t < nq; ++t) {
        bool any = false;
        float m = -INFINITY;
        for (int j = 0; j < nd; ++j) {
            if (keep && !(*keep)[(size_t)j]) continue;
            float dot = 0.0f;
            for (int b = 0; b < W / 16; ++b)
                for (int c = 0; c < 4; ++c)
                    for (int g = 0; g < 4; ++g) dot = fmaf(D[(size_t)j * W + 16 * b + 4 * g + c], Q[(size_t)t * W + 16 * b + 4 * g + c], dot);
            const bool greater = dot > m || (dot == m && std::signbit(m) && !std::signbit(dot));  // -0 < +0
            if (!any || greater) m = dot;
            any = true;
        }
        volatile float r = acc + m;
        acc = r;
    }
    return acc;
}

static float run(const std::vector<float>& Q, int nq, const std::vector<float>& D, int nd, const std::vector<unsigned char>* keep, int W) {
    // exact-size heap copies: an access past nq * W, nd * W or nd is the sanitizer's to report
    std::vector<float> q(Q.begin(), Q.begin() + (size_t)nq * W), d(D.begin(), D.begin() + (size_t)nd * W);
    std::vector<unsigned char> k;
    if (keep) k.assign(keep->begin(), keep->begin() + nd);
    return maxsim_score_seq(q.data(), nq, d.data(), nd, keep ? k.data() : nullptr, W);
}

int main() {
    {   // the key: order and round trip over the values that matter
        const float vals[] = {-INFINITY, -3.0f, -1e-38f, -0.0f, 0.0f, 1e-38f, 2.5f, INFINITY};
        for (int i = 0; i + 1 < 8; ++i)
            if (!(maxsim_key(vals[i]) < maxsim_key(vals[i + 1]))) {
                ++failures;
                std::printf("FAIL key order at %d\n", i);
            }
        for (float v : vals) expect("key round trip", maxsim_unkey(maxsim_key(v)), v);
        if (maxsim_key(-INFINITY) != MAXSIM_KEY_NONE) {
            ++failures;
            std::printf("FAIL MAXSIM_KEY_NONE\n");
        }
    }
    {   // signed zeros: a document of -0 dots and one +0 dot takes +0 wherever it stands; -0 alone stays -0 in the key, and +0 + -0 = +0
        const int W = 16;
        std::vector<float> Q((size_t)W, 0.0f), D((size_t)3 * W, 0.0f);
        Q[0] = 1.0f;
        D[0] = -0.0f;              // token 0: dot = fma(-0, 1, +0) = +0 ... the chain starts from +0, so a -0 product cannot make -0
        expect("zeros", run(Q, 1, D, 3, nullptr, W), 0.0f);
        expect("zeros plain", plain(Q, 1, D, 3, nullptr, W), 0.0f);
    }
    {   // ties and negative-only documents; the order of the document tokens does not matter
        const int W = 16;
        std::vector<float> Q((size_t)2 * W, 0.0f), D((size_t)4 * W, 0.0f), R((size_t)4 * W, 0.0f);
        Q[0] = 1.0f;
        Q[W + 1] = 1.0f;
        const float d0[4] = {-2.0f, -0.5f, -0.5f, -7.0f}, d1[4] = {-1.0f, -1.0f, -3.0f, -1.0f};
        for (int j = 0; j < 4; ++j) {
            D[(size_t)j * W] = d0[j];
            D[(size_t)j * W + 1] = d1[j];
            R[(size_t)(3 - j) * W] = d0[j];
            R[(size_t)(3 - j) * W + 1] = d1[j];
        }
        expect("negative only", run(Q, 2, D, 4, nullptr, W), -1.5f);
        expect("negative only, reversed", run(Q, 2, R, 4, nullptr, W), -1.5f);
        std::vector<unsigned char> keep = {1, 0, 0, 1};
        expect("keep mask", run(Q, 2, D, 4, &keep, W), -3.0f);
        std::vector<unsigned char> none = {0, 0, 0, 0};
        expect("nothing kept", run(Q, 2, D, 4, &none, W), -INFINITY);
    }
    // random vectors on a coarse grid (ties happen) against the plain restatement
    uint64_t z = 2024;
    auto rnd = [&] {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((int)(z >> 40) % 33 - 16) / 8.0f;
    };
    for (int W : {16, 96, 128})
        for (int nq : {1, 17, 32, 128})
            for (int nd : {1, 15, 16, 17, 300}) {
                std::vector<float> Q((size_t)nq * W), D((size_t)nd * W);
                for (float& v : Q) v = rnd();
                for (float& v : D) v = rnd();
                std::vector<unsigned char> keep((size_t)nd);
                for (int j = 0; j < nd; ++j) keep[(size_t)j] = (unsigned char)(j == nd / 2 || ((z >> (j % 48)) & 1));
                expect("random", run(Q, nq, D, nd, nullptr, W), plain(Q, nq, D, nd, nullptr, W));
                expect("random, keep", run(Q, nq, D, nd, &keep, W), plain(Q, nq, D, nd, &keep, W));
            }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
