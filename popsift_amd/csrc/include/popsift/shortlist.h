/* popsift::Vocabulary -- which view pairs to match: a visual vocabulary trained on the descriptors of a set of views, a bag
 * of words per view, and the k most similar views per view as the edge list that FeaturesDev::matchPairsGraph,
 * estimate*Graph, matchPairsGuidedGraph and buildTracks take (include/popsift_hip.h, "WHICH PAIRS TO MATCH":
 * psx_vocab_train_u8, psx_bow_u8, psx_shortlist_views).  The reference has no counterpart; AliceVision answers the same
 * question in its image-matching step before feature matching.
 * popsift::ViewDatabase -- the same question for views that arrive one at a time: a growing collection of stored views and
 * the k most similar of them per arriving view ("QUERY A DATABASE OF VIEWS": psx_bow_quantize_dev, psx_shortlist_query). */
#pragma once

#include "features.h"

#include <string>
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

    /// The vocabulary as a file (popsift/vocabulary_file.h: magic, version, words, dimension, the bytes, an FNV-1a checksum):
    /// training is the one step a deployment does once and stores.  save throws std::runtime_error for an empty vocabulary
    /// or a file that cannot be written; load for one that cannot be read, is short, has a wrong magic, version or
    /// dimension, words outside [2, 65536] or a checksum that does not match.  A loaded vocabulary gives the bags the
    /// saved one gave; its info() is empty.
    void save( const std::string& path ) const;
    static Vocabulary load( const std::string& path );

    /// Takes `words` words of 128 bytes as the vocabulary (trained elsewhere, or kept by the caller); info() is emptied.
    /// Throws std::runtime_error for a null pointer or words outside [2, 65536].
    void assign( const unsigned char* bytes, int words );

    int wordCount( ) const { return (int)( _words.size() / 128 ); }
    const std::vector<unsigned char>& words( ) const { return _words; }
    const VocabularyInfo& info( ) const { return _info; }
};

/// What ViewDatabase::query returns: one list per query view
struct QueryResult
{
    int                   k = 0;
    int                   edge_base = 0;  ///< the `left` of query i's edges is edge_base + i
    std::vector<int>      neighbours;   ///< queries * k: stored views by (score descending, index ascending), unused entries -1
    std::vector<unsigned> scores;       ///< queries * k: their scores, unused entries 0
    std::vector<ViewEdge> edges;        ///< { edge_base + i, neighbour }, grouped by left in list order: not sorted by right, not deduplicated
    /// the edges as FeaturesDev::matchPairsGraph and the calls after it take them
    std::vector<std::pair<int,int>> pairs() const;
};

/// A growing collection of views to rank new views against (include/popsift_hip.h, "QUERY A DATABASE OF VIEWS":
/// psx_bow_quantize_dev, psx_shortlist_query).  It owns the quantised bags of the stored views in device memory and the
/// document frequencies on the host; a view's row depends on nothing but the view, so adding views never touches the rows
/// already stored, and a query costs one row of scores per query view, not all pairs again.  At most 1 048 576 views.
/// Not kept: sparse bags or an inverted file, a vocabulary tree, removing views, persisting the database itself, float
/// descriptors.  Not thread safe; not copyable.
class ViewDatabase
{
    Vocabulary       _voc;
    int              _device;
    int              _capacity;
    int              _size = 0;
    void*            _q = nullptr;       // capacity x words uint16, device memory
    std::vector<int> _df;                // per word: the stored views that contain it

    QueryResult run( const void* d_query_q, int n, int k, unsigned min_score, int self_base, const int* limits, int edge_base ) const;

public:
    /// Throws std::runtime_error for an empty vocabulary, a capacity outside [1, 1 048 576] or no device memory.
    ViewDatabase( const Vocabulary& vocabulary, int device, int capacity );
    ~ViewDatabase( );
    ViewDatabase( const ViewDatabase& ) = delete;
    ViewDatabase& operator=( const ViewDatabase& ) = delete;

    /// Stores `views` behind the views already there (Vocabulary::bagOfWords, then psx_bow_quantize_dev); returns the index
    /// of the first.  Throws when the capacity would be exceeded (nothing is stored then) or a call fails.
    int add( const std::vector<FeaturesDev*>& views );

    /// The k stored views most like each of `views`, which are not stored: scores under weights() of at least min_score
    /// (and above 0).  The edges carry edge_base = size(): they index an array of the stored views followed by `views`.
    QueryResult query( const std::vector<FeaturesDev*>& views, int k, unsigned min_score = 0 ) const;

    /// The same for the stored views first .. first + count - 1, each without itself; with earlier_only every view is
    /// ranked against the views stored before it alone -- the loop-closure form.  edge_base = first.
    QueryResult queryStored( int first, int count, int k, bool earlier_only ) const;

    int size( ) const { return _size; }
    int capacity( ) const { return _capacity; }
    const Vocabulary& vocabulary( ) const { return _voc; }
    /// psx_bow_weights of the stored views' document frequencies: what the next query scores with
    std::vector<int> weights( ) const;
};

} // namespace popsift
