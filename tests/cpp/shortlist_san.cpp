// shortlist_san.cpp -- the host references of the view shortlist (popsift_amd/csrc/hip/bow_rule.h, bow_plan.h) as a
// stand-alone program under -fsanitize=address,undefined: the hand example of tests/test_shortlist_cpu.py and the capacity
// cuts, on arrays that are exactly as large as the contract says.  No HIP, no device.
#include "bow_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::vector<unsigned char> rows_of(const std::vector<int>& first_bytes)
{
    std::vector<unsigned char> r(first_bytes.size() * 128, 0);
    for (size_t i = 0; i < first_bytes.size(); i++) r[i * 128] = (unsigned char)first_bytes[i];
    return r;
}

int main()
{
    // two views, six rows that differ in their first byte only: 10 13 10 11 | 100 101; three words start as rows 0, 2, 4
    std::vector<unsigned char> v0 = rows_of({10, 13, 10, 11}), v1 = rows_of({100, 101});
    const unsigned char* sets[2] = {v0.data(), v1.data()};
    const int lens[2] = {4, 2};
    {
        // one iteration: words 0 and 1 are the same row, the tie goes to word 0 and word 1 stays empty and keeps its bytes;
        // {100, 101} average to 100.5, which rounds up
        std::vector<unsigned char> vocab(3 * 128, 0xA5);
        psx_vocab_opts o = {3, 1};
        psx_vocab_info info = {-1, -1, -1, -1, 77};
        CHECK(psx_vocab_train_host(sets, lens, 2, &o, vocab.data(), &info) == PSX_OK);
        CHECK(vocab[0] == 11 && vocab[128] == 10 && vocab[256] == 101);
        CHECK(info.iterations == 1 && info.changed == 6 && info.empty_words == 1 && info.reserved == 0 && info.inertia == 11);
        for (int w = 0; w < 3; w++)
            for (int k = 1; k < 128; k++) CHECK(vocab[(size_t)w * 128 + k] == 0);
    }
    std::vector<unsigned char> vocab(3 * 128, 0xA5);
    {
        // until nothing moves: three iterations, the last with no change
        psx_vocab_opts o = {3, 10};
        psx_vocab_info info = {-1, -1, -1, -1, 77};
        CHECK(psx_vocab_train_host(sets, lens, 2, &o, vocab.data(), &info) == PSX_OK);
        CHECK(vocab[0] == 12 && vocab[128] == 10 && vocab[256] == 101);
        CHECK(info.iterations == 3 && info.changed == 0 && info.empty_words == 0 && info.inertia == 3);
        // the errors leave the outputs alone
        psx_vocab_opts bad = {7, 10};                               // more words than rows
        psx_vocab_info keep = {-1, -1, -1, -1, 77};
        std::vector<unsigned char> untouched(7 * 128, 0xA5);
        CHECK(psx_vocab_train_host(sets, lens, 2, &bad, untouched.data(), &keep) == PSX_ERR_INVALID);
        CHECK(keep.iterations == -1 && untouched[0] == 0xA5);
    }
    {
        // row 3 (11) is as far from word 0 (12) as from word 1 (10): the lower word
        unsigned hist[6];
        int words[6];
        CHECK(psx_bow_host(vocab.data(), 3, sets, lens, 2, hist, words) == PSX_OK);
        const unsigned want_hist[6] = {2, 2, 0, 0, 0, 2};
        const int want_words[6] = {1, 0, 1, 0, 2, 2};
        for (int i = 0; i < 6; i++) CHECK(hist[i] == want_hist[i] && words[i] == want_words[i]);
        unsigned only[6];
        CHECK(psx_bow_host(vocab.data(), 3, sets, lens, 2, only, nullptr) == PSX_OK && only[5] == 2);
        const int none[2] = {0, 0};
        CHECK(psx_bow_host(vocab.data(), 3, sets, none, 2, only, nullptr) == PSX_OK && only[0] == 0 && only[5] == 0);
    }
    {
        // three views over two words; df = {3, 2}, weights {1, 10}, q = {32767, 32767} twice and {65535, 0}
        const unsigned hist[6] = {1, 1, 1, 1, 2, 0};
        const int df[2] = {3, 2};
        int weight[2] = {-1, -1};
        CHECK(psx_bow_weights_host(df, 2, 3, weight) == PSX_OK && weight[0] == 1 && weight[1] == 10);
        int nb[3], count = -1;
        unsigned sc[3];
        psx_view_edge edges[2];
        psx_shortlist_opts o = {1, 0};
        CHECK(psx_shortlist_host(hist, 3, 2, &o, nb, sc, edges, 2, &count) == PSX_OK);
        CHECK(count == 2 && nb[0] == 1 && nb[1] == 0 && nb[2] == 0);            // view 2 sees 0 and 1 alike: the lower
        CHECK(sc[0] == 360437u && sc[1] == 360437u && sc[2] == 32767u);
        CHECK(edges[0].left == 0 && edges[0].right == 1 && edges[1].left == 0 && edges[1].right == 2);
        o.flags = PSX_SHORTLIST_MUTUAL;
        psx_view_edge one[1];
        CHECK(psx_shortlist_host(hist, 3, 2, &o, nullptr, nullptr, one, 1, &count) == PSX_OK);
        CHECK(count == 1 && one[0].left == 0 && one[0].right == 1);
        // k above N - 1: every pair, unused entries -1 and 0; the capacity cuts
        psx_shortlist_opts all = {4, 0};
        int nb4[12];
        unsigned sc4[12];
        psx_view_edge e3[3];
        CHECK(psx_shortlist_host(hist, 3, 2, &all, nb4, sc4, e3, 3, &count) == PSX_OK && count == 3);
        CHECK(nb4[0] == 1 && nb4[1] == 2 && nb4[2] == -1 && nb4[3] == -1 && sc4[2] == 0 && nb4[8] == 0 && nb4[9] == 1 && nb4[10] == -1);
        CHECK(e3[2].left == 1 && e3[2].right == 2);
        psx_view_edge e2[2];
        CHECK(psx_shortlist_host(hist, 3, 2, &all, nullptr, nullptr, e2, 2, &count) == PSX_OK && count == 3);
        CHECK(e2[1].left == 0 && e2[1].right == 2);
        CHECK(psx_shortlist_host(hist, 3, 2, &all, nullptr, nullptr, nullptr, 0, &count) == PSX_OK && count == 3);
        count = -5;
        CHECK(psx_shortlist_host(hist, 3, 2, &all, nullptr, nullptr, nullptr, 1, &count) == PSX_ERR_INVALID && count == -5);
        psx_shortlist_opts bad = {0, 0};
        CHECK(psx_shortlist_host(hist, 3, 2, &bad, nullptr, nullptr, nullptr, 0, &count) == PSX_ERR_INVALID && count == -5);
    }
    if (failures == 0) std::printf("ALL OK\n");
    return failures == 0 ? 0 : 1;
}
