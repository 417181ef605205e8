// mmr_rule_check.cpp -- stand-alone check of semcode_amd/csrc/mmr_rule.h (the selection rule of the MMR search) on the CPU, meant
// to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Isemcode_amd/csrc scripts/mmr_rule_check.cpp -o mmr_rule_check
// It calls the rule the way sc_diag_mmr_select_host (sc_mmr.cpp) does -- heap scratch of exactly C entries, picked of exactly
// min(k, C) -- so that an index one past either end is an error, over the tie cases of tests/test_mmr_host.py and random
// symmetric matrices.  Exit status 0 and "ok" when every case gives the expected picks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mmr_rule.h"

static std::vector<int32_t> run(const std::vector<float>& rel, const std::vector<float>& G, int ldg, int k, float lambda) {
    const int C = (int)rel.size();
    std::vector<float> m((size_t)C);
    std::vector<unsigned char> taken((size_t)C);
    std::vector<int32_t> picked((size_t)(k < C ? k : C), -7);
    const int got = mmr_select_seq(rel.data(), G.data(), C, ldg, k, lambda, m.data(), taken.data(), picked.data());
    if (got != (int)picked.size()) {
        std::printf("FAIL: %d picks, expected %zu\n", got, picked.size());
        std::exit(1);
    }
    return picked;
}

static int failures = 0;
static void expect(const char* what, const std::vector<int32_t>& got, const std::vector<int32_t>& want) {
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: got", what);
    for (int v : got) std::printf(" %d", v);
    std::printf("\n");
}

// the definition again, written without the header: plain loops, products rounded through volatile
static std::vector<int32_t> plain(const std::vector<float>& rel, const std::vector<float>& G, int ldg, int k, float lambda) {
    const int C = (int)rel.size();
    const int steps = k < C ? k : C;
    std::vector<int32_t> picked;
    if (steps < 1) return picked;
    std::vector<char> taken((size_t)C, 0);
    picked.push_back(0);
    taken[0] = 1;
    volatile float mu = 1.0f - lambda;
    for (int t = 1; t < steps; ++t) {
        int best = -1;
        float bv = 0.0f;
        for (int i = 0; i < C; ++i) {
            if (taken[(size_t)i]) continue;
            float m = -INFINITY;
            for (int j : picked) m = G[(size_t)i * ldg + j] > m ? G[(size_t)i * ldg + j] : m;
            volatile float a = lambda * rel[(size_t)i];
            volatile float b = mu * m;
            const float v = a - b;
            if (best < 0 || v > bv) {
                best = i;
                bv = v;
            }
        }
        picked.push_back(best);
        taken[(size_t)best] = 1;
    }
    return picked;
}

int main() {
    {   // equal values walk up the indices
        std::vector<float> rel(9, 0.25f), G(81, 0.5f);
        for (float lambda : {0.0f, 0.3f, 1.0f}) expect("all equal", run(rel, G, 9, 9, lambda), {0, 1, 2, 3, 4, 5, 6, 7, 8});
    }
    {   // 2 and 5 tie on top
        std::vector<float> rel = {9, 1, 4, 1, 1, 4, 1}, G(49, 0.0f);
        expect("tie 2/5", run(rel, G, 7, 4, 0.5f), {0, 2, 5, 1});
        G[2 * 7 + 5] = G[5 * 7 + 2] = 8.0f;
        expect("tie 2/5, 5 redundant with 2", run(rel, G, 7, 7, 0.5f), {0, 2, 1, 3, 4, 6, 5});
    }
    {   // +0 and -0 are one value
        std::vector<float> rel = {1.0f, -0.0f, 0.0f}, G(9, 0.0f);
        expect("signed zeros", run(rel, G, 3, 3, 1.0f), {0, 1, 2});
    }
    {   // equal maxima in G
        std::vector<float> rel = {5, 4, 3, 2, 1};
        std::vector<float> G = {0, 1, 1, 1, 1, 1, 0, 1, 3, 3, 1, 1, 0, 3, 0.5f, 1, 3, 3, 0, 3, 1, 3, 0.5f, 3, 0};
        expect("equal maxima, lambda 0", run(rel, G, 5, 5, 0.0f), {0, 1, 2, 3, 4});
        expect("equal maxima, lambda 0.5", run(rel, G, 5, 5, 0.5f), {0, 1, 2, 3, 4});
    }
    {   // three roundings: a fused multiply-add would pick candidate 2 (tests/test_mmr_host.py)
        const float lambda = 4097.0f / 8192.0f;
        std::vector<float> rel = {8.0f, 3.0f, 4097.0f / 2048.0f}, G(9, 0.0f);
        G[0 * 3 + 1] = G[1 * 3 + 0] = 3.0f;
        G[0 * 3 + 2] = G[2 * 3 + 0] = 2.0f;
        expect("no fma", run(rel, G, 3, 2, lambda), {0, 1});
    }
    {   // k and C at their ends; ldg > C
        std::vector<float> one = {2.0f}, G1 = {0.0f, 7.0f};
        expect("C = 1", run(one, G1, 2, 5, 0.5f), {0});
        std::vector<float> rel = {3, 2, 1}, G(3 * 5, 0.0f);
        expect("k = 1", run(rel, G, 5, 1, 0.5f), {0});
    }
    // random symmetric matrices against the plain restatement, C up to the limit of the search
    uint64_t z = 12345;
    auto rnd = [&] {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((int)(z >> 40) % 2001 - 1000) / 64.0f;  // a coarse grid: ties happen
    };
    for (int C : {2, 17, 64, 128})
        for (float lambda : {0.0f, 0.5f, 1.0f}) {
            const int ldg = C + 3;
            std::vector<float> rel((size_t)C), G((size_t)C * ldg, 0.0f);
            for (float& r : rel) r = rnd();
            for (int i = 0; i < C; ++i)
                for (int j = i; j < C; ++j) G[(size_t)i * ldg + j] = G[(size_t)j * ldg + i] = rnd();
            for (int k : {1, C / 2 + 1, C, C + 4}) expect("random", run(rel, G, ldg, k, lambda), plain(rel, G, ldg, k, lambda));
        }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
