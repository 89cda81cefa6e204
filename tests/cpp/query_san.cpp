// query_san.cpp -- the host side of the database query (popsift_amd/csrc/hip/bow_rule.h, bow_plan.h) and the vocabulary file
// (popsift/vocabulary_file.h) as a stand-alone program under -fsanitize=address,undefined: a hand example, the capacity
// cuts and the refusals on arrays that are exactly as large as the contract says, a round trip of a vocabulary through a
// file and each malformed file.  No HIP, no device.  argv[1]: a directory to write the files in.
#include "bow_plan.h"
#include <popsift/vocabulary_file.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

namespace vf = popsift::vocabulary_file;

static std::string error_of(const std::vector<unsigned char>& file)
{
    try { vf::decode(file.data(), file.size()); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static void put_file(const std::string& path, const std::vector<unsigned char>& bytes)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != nullptr);
    if (f == nullptr) return;
    CHECK(std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size());
    std::fclose(f);
}

int main(int argc, char** argv)
{
    {
        // three views over two words, as in shortlist_san.cpp: {1, 1} twice and {2, 0}; df = {3, 2}, weights {1, 10}
        const unsigned hist[6] = {1, 1, 1, 1, 2, 0};
        unsigned short q[6];
        int df[2] = {0, 0};
        CHECK(psx_bow_quantize_host(hist, 2, 2, q, df) == PSX_OK);            // two views, then the third behind them
        CHECK(psx_bow_quantize_host(hist + 4, 1, 2, q + 4, df) == PSX_OK);
        CHECK(q[0] == 32767 && q[1] == 32767 && q[3] == 32767 && q[4] == 65535 && q[5] == 0 && df[0] == 3 && df[1] == 2);
        unsigned short only[2];
        CHECK(psx_bow_quantize_host(hist + 4, 1, 2, only, nullptr) == PSX_OK && only[0] == 65535);
        CHECK(psx_bow_quantize_host(hist, 1, 0, only, nullptr) == PSX_ERR_INVALID && only[0] == 65535);
        int weight[2];
        CHECK(psx_bow_weights_host(df, 2, 3, weight) == PSX_OK && weight[0] == 1 && weight[1] == 10);
        // the database as its own queries: what psx_shortlist_host gives, and the edges in list order
        psx_query_opts o = {1, 0, 0, 0, 0u, 0};
        int nb[3], count = -1;
        unsigned sc[3];
        psx_view_edge edges[3];
        CHECK(psx_shortlist_query_host(q, 3, q, 3, 2, weight, nullptr, &o, nb, sc, edges, 3, &count) == PSX_OK);
        CHECK(count == 3 && nb[0] == 1 && nb[1] == 0 && nb[2] == 0 && sc[0] == 360437u && sc[2] == 32767u);
        CHECK(edges[0].left == 0 && edges[0].right == 1 && edges[1].left == 1 && edges[1].right == 0 && edges[2].left == 2 && edges[2].right == 0);
        // one arriving view {2, 0} against the first two, edges behind the database; k above n_db
        psx_query_opts arrive = {4, 0, -1, 2, 0u, 0};
        int nb4[4];
        unsigned sc4[4];
        psx_view_edge e2[2];
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, nullptr, &arrive, nb4, sc4, e2, 2, &count) == PSX_OK && count == 2);
        CHECK(nb4[0] == 0 && nb4[1] == 1 && nb4[2] == -1 && nb4[3] == -1 && sc4[0] == 32767u && sc4[1] == 32767u && sc4[2] == 0u);
        CHECK(e2[0].left == 2 && e2[0].right == 0 && e2[1].left == 2 && e2[1].right == 1);
        // a limit, a least score, the capacity cuts
        const int limit[1] = {1};
        psx_view_edge e1[1];
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, limit, &arrive, nullptr, nullptr, e1, 1, &count) == PSX_OK && count == 1);
        CHECK(e1[0].left == 2 && e1[0].right == 0);
        arrive.min_score = 32768u;
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, nullptr, &arrive, nb4, nullptr, nullptr, 0, &count) == PSX_OK && count == 0);
        CHECK(nb4[0] == -1);
        arrive.min_score = 0u;
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, nullptr, &arrive, nullptr, nullptr, e1, 1, &count) == PSX_OK && count == 2);
        CHECK(e1[0].right == 0);
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, nullptr, &arrive, nullptr, nullptr, nullptr, 0, &count) == PSX_OK && count == 2);
        // an empty database writes every entry as unused; no query writes nothing
        nb4[0] = 7;
        CHECK(psx_shortlist_query_host(nullptr, 0, q + 4, 1, 2, weight, nullptr, &arrive, nb4, sc4, nullptr, 0, &count) == PSX_OK && count == 0);
        CHECK(nb4[0] == -1 && nb4[3] == -1 && sc4[3] == 0u);
        nb4[0] = 7;
        CHECK(psx_shortlist_query_host(q, 2, nullptr, 0, 2, weight, nullptr, &arrive, nb4, sc4, nullptr, 0, &count) == PSX_OK && count == 0 && nb4[0] == 7);
        // the refusals leave the outputs alone
        count = -5;
        const int heavy[2] = {1, 1024}, low[1] = {3};
        psx_query_opts bad = arrive;
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, heavy, nullptr, &arrive, nb4, sc4, nullptr, 0, &count) == PSX_ERR_INVALID);
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, low, &arrive, nb4, sc4, nullptr, 0, &count) == PSX_ERR_INVALID);
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, nullptr, &arrive, nb4, sc4, nullptr, 1, &count) == PSX_ERR_INVALID);
        bad.flags = 1;
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, nullptr, &bad, nb4, sc4, nullptr, 0, &count) == PSX_ERR_INVALID);
        bad = arrive; bad.self_base = 2;
        CHECK(psx_shortlist_query_host(q, 2, q + 4, 1, 2, weight, nullptr, &bad, nb4, sc4, nullptr, 0, &count) == PSX_ERR_INVALID);
        CHECK(count == -5 && nb4[0] == 7);
        // the plan
        psx_query_plan p = {-1, -1, -1, -1};
        CHECK(psx_query_plan_host(130, 5, 33, 70, &p) == PSX_OK && p.blocks == 3 && p.keys_per_block == 64 && p.partial_keys == 960);
        CHECK(p.scratch_bytes == 144 + 32 + 8 * 960 + 4 * (2 * 2 + 2));
        CHECK(psx_query_plan_host(PSX_QUERY_MAX_VIEWS, 129, 8, 64, &p) == PSX_ERR_INVALID && p.blocks == 3);
        // the keys: 20 index bits under a score of 26
        const unsigned long long key = psx_query_key(65535u * 1023u, PSX_QUERY_MAX_VIEWS - 1);
        CHECK(key < (1ULL << 46) && psx_query_key_score(key) == 65535u * 1023u && psx_query_key_view(key) == PSX_QUERY_MAX_VIEWS - 1);
        CHECK(psx_query_key(7u, 3) > psx_query_key(7u, 4) && psx_query_key(8u, 4) > psx_query_key(7u, 3) && psx_query_key_view(psx_query_key(7u, 0)) == 0);
    }
    {
        // the vocabulary file: a round trip in memory and through a file, then every malformed form
        std::vector<unsigned char> words(3 * 128);
        for (size_t i = 0; i < words.size(); i++) words[i] = (unsigned char)(i * 7 + i / 128);
        const std::vector<unsigned char> file = vf::encode(words.data(), 3);
        CHECK(file.size() == 20 + 3 * 128 + 8);
        CHECK(vf::decode(file.data(), file.size()) == words);
        if (argc > 1) {
            const std::string dir = argv[1];
            vf::write(dir + "/three.psxvocab", words.data(), 3);
            CHECK(vf::read(dir + "/three.psxvocab") == words);
            std::vector<unsigned char> cut(file.begin(), file.end() - 1);
            put_file(dir + "/cut.psxvocab", cut);
            std::string e;
            try { vf::read(dir + "/cut.psxvocab"); } catch (const std::runtime_error& x) { e = x.what(); }
            CHECK(has(e, "shorter"));
            e.clear();
            try { vf::read(dir + "/missing.psxvocab"); } catch (const std::runtime_error& x) { e = x.what(); }
            CHECK(has(e, "cannot open"));
            // the largest vocabulary there is
            std::vector<unsigned char> big((size_t)65536 * 128);
            for (size_t i = 0; i < big.size(); i++) big[i] = (unsigned char)(i % 251);
            vf::write(dir + "/big.psxvocab", big.data(), 65536);
            CHECK(vf::read(dir + "/big.psxvocab") == big);
        }
        CHECK(has(error_of(std::vector<unsigned char>()), "too short"));
        CHECK(has(error_of(std::vector<unsigned char>(file.begin(), file.begin() + 19)), "too short"));
        CHECK(has(error_of(std::vector<unsigned char>(file.begin(), file.begin() + 20)), "shorter"));
        CHECK(has(error_of(std::vector<unsigned char>(file.begin(), file.end() - 1)), "shorter"));
        std::vector<unsigned char> f = file;
        f.push_back(0);
        CHECK(has(error_of(f), "longer"));
        f = file; f[0] = 'Q';
        CHECK(has(error_of(f), "magic"));
        f = file; f[8] = 2;
        CHECK(has(error_of(f), "version"));
        f = file; f[16] = 64;
        CHECK(has(error_of(f), "dimension"));
        f = file; f[12] = 1;                                                  // one word
        CHECK(has(error_of(f), "words outside"));
        f = file; f[12] = 1; f[14] = 1;                                       // 65537 words
        CHECK(has(error_of(f), "words outside"));
        f = file; f[12] = 4;                                                  // more words than bytes
        CHECK(has(error_of(f), "shorter"));
        f = file; f[100] ^= 1;
        CHECK(has(error_of(f), "checksum"));
        f = file; f[f.size() - 1] ^= 0x80;
        CHECK(has(error_of(f), "checksum"));
        std::string e;
        try { vf::encode(words.data(), 1); } catch (const std::runtime_error& x) { e = x.what(); }
        CHECK(has(e, "words outside"));
        CHECK(vf::fnv1a(reinterpret_cast<const unsigned char*>("a"), 1) == 0xaf63dc4c8601ec8cULL);          // the published test vector
    }
    if (failures == 0) std::printf("ALL OK\n");
    return failures == 0 ? 0 : 1;
}
