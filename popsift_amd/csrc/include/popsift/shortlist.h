/* popsift::Vocabulary -- which view pairs to match: a visual vocabulary trained on the descriptors of a set of views, a bag
 * of words per view, and the k most similar views per view as the edge list that FeaturesDev::matchPairsGraph,
 * estimate*Graph, matchPairsGuidedGraph and buildTracks take (include/popsift_hip.h, "WHICH PAIRS TO MATCH":
 * psx_vocab_train_u8, psx_bow_u8, psx_shortlist_views).  The reference has no counterpart; AliceVision answers the same
 * question in its image-matching step before feature matching. */
#pragma once

#include "features.h"

#include <utility>
#include <vector>

namespace popsift {

/// One pair of views to match, left < right: indices into the `views` the bags were made from
struct ViewEdge
{
    int left;
    int right;
};

/// What Vocabulary::train reports about its last iteration (psx_vocab_info)
struct VocabularyInfo
{
    int                iterations  = 0;   ///< iterations run: fewer than asked for when no row changed its word
    int                changed     = 0;   ///< rows whose word changed in the last assignment
    int                empty_words = 0;   ///< words without a row in the last assignment
    unsigned long long inertia     = 0;   ///< sum of squared distances of the last assignment
};

/// One histogram row per view: counts[ v * words + w ] = the descriptors of view v assigned to word w
struct BagsOfWords
{
    int                   views = 0;
    int                   words = 0;
    std::vector<unsigned> counts;
};

/// What Vocabulary::shortlist returns
struct Shortlist
{
    int                   k = 0;
    std::vector<int>      neighbours;   ///< views * k: the list of view v at [ v*k, v*k + k ), unused entries -1
    std::vector<unsigned> scores;       ///< views * k: their scores, unused entries 0
    std::vector<ViewEdge> edges;        ///< sorted by (left, right), each pair once
    /// the edges as FeaturesDev::matchPairsGraph and the calls after it take them
    std::vector<std::pair<int,int>> pairs() const;
};

class Vocabulary
{
    std::vector<unsigned char> _words;   // words x 128 bytes
    VocabularyInfo             _info;

public:
    /// Integer k-means over the byte form of the views' descriptors (float arrays quantised on the device by
    /// psx_quantize_desc, as FeaturesDev::matchBytes does): `words` words, at most `iterations` iterations.  A null entry
    /// counts as an empty view.  Throws std::runtime_error for views on different devices, fewer descriptors than words,
    /// words outside [2, 65536], iterations < 1, or a failing call.
    void train( const std::vector<FeaturesDev*>& views, int words, int iterations );

    /// The bags of words of `views` under this vocabulary in ONE device call (psx_bow_u8).  Throws when the vocabulary is
    /// empty, for views on different devices, or a failing call.
    BagsOfWords bagOfWords( const std::vector<FeaturesDev*>& views ) const;

    /// The k most similar views of every view by idf-weighted histogram intersection, and the edge list; with `mutual`
    /// only the pairs in which each view lists the other.  At most 4096 views.  Runs on `device`.
    static Shortlist shortlist( const BagsOfWords& bags, int k, bool mutual = false, int device = 0 );

    int wordCount( ) const { return (int)( _words.size() / 128 ); }
    const std::vector<unsigned char>& words( ) const { return _words; }
    const VocabularyInfo& info( ) const { return _info; }
};

} // namespace popsift
