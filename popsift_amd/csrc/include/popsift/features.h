// popsift/features.h -- result types handed to the caller.
//
// Same public surface as the reference (features.h:23-122): Feature (coordinates in input-image
// pixels, up to 4 orientations, pointers into the owning object's descriptor array),
// FeaturesBase, FeaturesHost (alias Features) and FeaturesDev.
#pragma once

#include "sift_constants.h"

#include <iostream>
#include <utility>
#include <vector>

namespace popsift {

struct Descriptor; // float features[128]

struct Feature
{
    int         debug_octave;
    float       xpos;
    float       ypos;
    /// scale
    float       sigma;
    /// number of valid entries in orientation[] / desc[]
    int         num_ori;
    float       orientation[ORIENTATION_MAX_COUNT];
    Descriptor* desc[ORIENTATION_MAX_COUNT];

    void print( std::ostream& ostr, bool write_as_uchar ) const;
};

std::ostream& operator<<( std::ostream& ostr, const Feature& feature );

class FeaturesBase
{
    int _num_ext;
    int _num_ori;

public:
    FeaturesBase( );
    virtual ~FeaturesBase( );

    inline int  size() const                { return _num_ext; }
    inline int  getFeatureCount() const     { return _num_ext; }
    inline int  getDescriptorCount() const  { return _num_ori; }

    inline void setFeatureCount( int num_ext )    { _num_ext = num_ext; }
    inline void setDescriptorCount( int num_ori ) { _num_ori = num_ori; }
};

/// Host-resident result: arrays owned by the object.  Objects produced by PopSift hold pooled buffers
/// (the descriptor array is the pinned buffer the GPU wrote the descriptors into: no copy); they go back
/// to a process-wide pool when the object is deleted.
class FeaturesHost : public FeaturesBase
{
    Feature*     _ext;
    Descriptor*  _ori;       // byte results: the no x 128 bytes (getDescriptorBytes)
    size_t       _ext_cap;   // bytes; 0: _ext came from posix_memalign
    size_t       _ori_cap;   // bytes; 0: _ori came from posix_memalign
    bool         _bytes;     // Config::ByteDescriptors: _ori holds bytes, Feature::desc[] are nullptr
    std::vector<int> _desc_idx;   // byte results: descriptor row of (feature, orientation), 4 per feature (psx_feature::desc_idx)
    std::vector<int> _src_idx;    // results at caller-supplied keypoints: input record of every feature; empty for detector jobs

public:
    FeaturesHost( );
    FeaturesHost( int num_ext, int num_ori );
    ~FeaturesHost( ) override;

    typedef Feature*       F_iterator;
    typedef const Feature* F_const_iterator;

    inline F_iterator       begin()       { return _ext; }
    inline F_const_iterator begin() const { return _ext; }
    inline F_iterator       end()         { return &_ext[size()]; }
    inline F_const_iterator end() const   { return &_ext[size()]; }

    void reset( int num_ext, int num_ori );
    /// kept for source compatibility: results arrive in pooled pinned buffers (DMA download or zero-copy export), nothing to pin per image
    void pin( );
    void unpin( );

    inline Feature*    getFeatures()    { return _ext; }
    /// float descriptors; nullptr for a byte result (no caller may read bytes as floats)
    inline Descriptor* getDescriptors() { return _bytes ? nullptr : _ori; }

    /// byte results (Config::ByteDescriptors): getDescriptorCount() rows of 128 bytes; nullptr for a float result
    inline bool hasByteDescriptors() const { return _bytes; }
    inline const unsigned char* getDescriptorBytes() const { return _bytes ? reinterpret_cast<const unsigned char*>( _ori ) : nullptr; }
    /// the 128 bytes of orientation `ori` of feature `feature`; nullptr for a float result or an orientation without descriptor
    const unsigned char* descriptorBytes( int feature, int ori ) const;
    /// row of (feature, ori) in the descriptor array, -1 when it has none (both formats)
    int descriptorIndex( int feature, int ori ) const;

    void print( std::ostream& ostr, bool write_as_uchar ) const;

    /// internal (PopSift): take ownership of pooled buffers (see host_pool.h); caps in bytes
    void adopt( int num_ext, int num_ori, Feature* ext, size_t ext_cap, Descriptor* ori, size_t ori_cap );
    /// internal (PopSift): the same for a byte result; bytes = num_ori x 128, desc_idx = 4 rows per feature
    void adoptBytes( int num_ext, int num_ori, Feature* ext, size_t ext_cap, unsigned char* bytes, size_t bytes_cap,
                     std::vector<int>&& desc_idx );
    /// internal (PopSift): pageable arrays for a byte result (the pinned-pool limit is exceeded)
    void resetBytes( int num_ext, int num_ori );
    inline unsigned char* byteStorage() { return _bytes ? reinterpret_cast<unsigned char*>( _ori ) : nullptr; }
    inline std::vector<int>& byteIndex() { return _desc_idx; }

    /// results of a job enqueued with keypoints: getSourceIndices()[i] = index of the input record feature i came from
    /// (records the placement rule dropped are absent); empty for detector jobs
    inline const std::vector<int>& getSourceIndices() const { return _src_idx; }
    /// internal (PopSift)
    inline std::vector<int>& sourceIndices() { return _src_idx; }

protected:
    friend class Pyramid;
    void release( );
};

using Features = FeaturesHost;

std::ostream& operator<<( std::ostream& ostr, const FeaturesHost& feature );

/// How FeaturesDev::matchPairs filters: the pair rule of psx_match_pairs (include/popsift_hip.h, "matches as data")
struct MatchOptions
{
    float ratio  = 0.8f;    ///< keep a pair iff distance / second_distance < ratio (float32); INFINITY: no ratio test
    bool  mutual = false;   ///< cross-check: the right descriptor's best left descriptor must be this one
    bool  bytes  = false;   ///< quantise both sides (psx_quantize_desc) and run the exact integer matcher, as matchBytes
};

/// What FeaturesDev::matchPairsGuided knows about where a match can lie: the guide of psx_match_pairs_guided
/// (include/popsift_hip.h, "guided matching").  Positions are Feature::xpos / ypos, in input-image units.
struct MatchGuide
{
    enum Kind { None = 0, Homography = 1, Epipolar = 2 } kind;   ///< m = H: right point within tol of H * left point
                                                       ///< (identity H: a search window); m = F: within tol of the line
                                                       ///< F * left point; None: matchPairsGuidedMany skips the set
                                                       ///< (matchPairsGuided refuses it)
    float m[9];                                        ///< row major
    float tol;                                         ///< pixels, finite and >= 0

    /// the guide of a set that FeaturesDev::matchPairsGuidedMany skips: kind None, a zero matrix, tol 0
    static MatchGuide none() { MatchGuide g; g.kind = None; for( int k = 0; k < 9; k++ ) g.m[k] = 0.0f; g.tol = 0.0f; return g; }
};

/// One correspondence of FeaturesDev::matchPairs / matchPairsGuided
struct Match
{
    int   left_feature, right_feature;          ///< indices into the two feature arrays (via the reverse maps)
    int   left_descriptor, right_descriptor;    ///< indices into the two descriptor arrays
    float distance, second_distance;            ///< squared; byte distances converted (exact), +inf: no second neighbour
};

/// How FeaturesDev::estimateHomography, estimateFundamental, estimateAffine and estimateSimilarity run: the options of
/// psx_ransac_homography, psx_ransac_fundamental, psx_ransac_affine and psx_ransac_similarity (include/popsift_hip.h,
/// "geometric verification")
struct RansacOptions
{
    float    tol        = 2.0f;   ///< inlier tolerance in pixels, finite and >= 0
    int      hypotheses = 1024;   ///< 1 .. 65536
    unsigned seed       = 0;      ///< the same seed on the same matches gives the same result, bit for bit
    bool     refit      = true;   ///< refit the winner over its inliers (kept iff it does not lose inliers)
};

/// What FeaturesDev::estimateHomography returns
struct HomographyEstimate
{
    MatchGuide         guide;            ///< Homography, the estimated matrix (this -> other), tol = RansacOptions::tol:
                                         ///< ready for matchPairsGuided
    std::vector<Match> inliers;          ///< the matches that pass under the matrix, in input order
    int                best;             ///< the winning hypothesis; -1: no model (fewer than 4 matches, or all degenerate)
    int                sample_inliers;   ///< inliers of the winning 4-point model
    bool               refit_kept;       ///< the refit model replaced it
};

/// What FeaturesDev::estimateFundamental returns: the same fields; guide is Epipolar, the estimated fundamental matrix
/// (this -> other); the sample has 8 points and best = -1 stands for fewer than 8 matches or no usable model
typedef HomographyEstimate FundamentalEstimate;
/// FeaturesDev::estimateAffine and estimateSimilarity return a HomographyEstimate: guide is Homography, a matrix whose last
/// row is exactly (0, 0, 1); the sample has 3 / 2 points and best = -1 stands for fewer matches than that or no finite model

/// How FeaturesDev::buildTracks runs: the options of psx_tracks_graph (include/popsift_hip.h, "TRACKS FROM A LIST OF VIEW PAIRS")
struct TrackOptions
{
    int  min_views      = 2;       ///< a track has members in at least this many views, >= 2
    bool keep_conflicts = false;   ///< keep the components that have two members in one view
};

/// One member of a track: a descriptor row of a view
struct TrackMember
{
    int view;          ///< index into `views`
    int descriptor;    ///< index into that view's descriptor array
};

/// What FeaturesDev::buildTracks returns: track t owns members[ starts[t] .. starts[t+1] ), tracks ordered by their
/// smallest (view, descriptor), members by view, then by descriptor
struct Tracks
{
    std::vector<int>         starts;         ///< n_tracks + 1 offsets into members
    std::vector<TrackMember> members;
    std::vector<int>         labels;         ///< labels[ view_offsets[v] + d ]: the track of descriptor d of view v, -1: in none
    std::vector<int>         view_offsets;   ///< views.size() + 1: the exclusive prefix sum of the views' descriptor counts
    int n_tracks, n_members;                 ///< starts.size() - 1 and members.size()
    int components;                          ///< connected components of 2 or more members
    int conflicts;                           ///< those with two members in one view
    int too_few_views;                       ///< those in fewer than min_views views
    int joined_records;                      ///< the matches that are not self-loops
};

/// Device-resident result (MatchingMode): arrays live in HBM of the extracting device.
class FeaturesDev : public FeaturesBase
{
    Feature*     _ext;   // device: psx_feature records (indices instead of pointers)
    Descriptor*  _ori;   // device
    int*         _rev;   // device: descriptor -> extremum
    int          _device;

    // every wrapper below states its call as views + edge list (features.cpp): form = one pair, star or edge list
    static int checkViews( const char* who, int form, const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                           size_t given, const char* what );
    static std::vector<std::vector<Match>> matchLists( const char* who, int form, const std::vector<FeaturesDev*>& views,
                                                       const std::vector<std::pair<int,int>>& edges, const std::vector<MatchGuide>* guides,
                                                       const MatchOptions& opts, const char* wrong_format );
    enum RansacModel { ModelHomography, ModelFundamental, ModelAffine, ModelSimilarity };   // what estimate() fits
    HomographyEstimate estimate( const char* who, RansacModel model, FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts );
    std::vector<HomographyEstimate> estimateMany( const char* who, RansacModel model, const std::vector<FeaturesDev*>& others,
                                                  const std::vector<std::vector<Match>>& matches, const RansacOptions& opts );
    static std::vector<HomographyEstimate> estimateGraph( const char* who, RansacModel model, const std::vector<FeaturesDev*>& views,
                                                          const std::vector<std::pair<int,int>>& edges,
                                                          const std::vector<std::vector<Match>>& matches, const RansacOptions& opts );

public:
    FeaturesDev( );
    FeaturesDev( int num_ext, int num_ori );
    ~FeaturesDev( ) override;

    void reset( int num_ext, int num_ori );

    /// brute-force 2-NN matcher of the reference (features.cu:160-304): prints one accept/reject line
    /// per descriptor of *this, as the reference's show_distance does
    void match( FeaturesDev* other );
    /// the same on bytes: both float arrays quantised on the device (psx_quantize_desc), then the exact integer
    /// matcher psx_match_u8; prints the same accept / reject lines as match()
    void matchBytes( FeaturesDev* other );
    /// the matches as data: the pairs (descriptor of *this, its best descriptor of *other) that pass the ratio test
    /// and, with MatchOptions::mutual, the cross-check, in ascending left descriptor; prints nothing.  Throws
    /// std::runtime_error for a null argument, objects on different devices, or a failing call.
    std::vector<Match> matchPairs( FeaturesDev* other, const MatchOptions& opts = MatchOptions() );
    /// matchPairs with every descriptor's search restricted to the descriptors of the other side that the guide admits
    /// (this = left, other = right; the cross-check runs on the same relation).  The positions are those of the
    /// features the descriptors belong to (psx_desc_positions on each object's own arrays).  Throws as matchPairs,
    /// and for an invalid guide.
    std::vector<Match> matchPairsGuided( FeaturesDev* other, const MatchGuide& guide, const MatchOptions& opts = MatchOptions() );
    /// matchPairs against many objects in ONE device call (psx_match_pairs_many_u8: one synchronisation, a number of
    /// launches that does not grow with others.size()): element k equals matchPairs( others[k], opts ).  Byte
    /// descriptors only -- every side is quantised once on the device, as matchPairs does with MatchOptions::bytes.
    /// Throws as matchPairs for a null entry or an object on another device, and for opts.bytes == false.
    std::vector<std::vector<Match>> matchPairsMany( const std::vector<FeaturesDev*>& others, const MatchOptions& opts );
    /// matchPairs over a LIST OF VIEW PAIRS in ONE device call (psx_match_pairs_graph_u8: one synchronisation, a number of
    /// launches that grows neither with edges.size() nor with views.size()): edges[e] = (left, right) indexes `views`,
    /// element e equals views[left]->matchPairs( views[right], opts ) field by field, in the order of the list -- which
    /// may name a pair twice, in both orders, or a view against itself.  Byte descriptors only; every referenced view is
    /// quantised once for the whole call.  Throws as matchPairsMany (a null referenced entry, views on different devices,
    /// opts.bytes == false), and for an edge index outside `views`.
    static std::vector<std::vector<Match>> matchPairsGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                            const MatchOptions& opts );
    /// matchPairsMany on the objects' FLOAT descriptors (psx_match_pairs_many): no quantisation, no copies; element k
    /// equals matchPairs( others[k], opts ) field by field, and the estimate*Many functions accept the lists unchanged.
    /// Throws as matchPairs for a null entry or an object on another device, and for opts.bytes == true (use
    /// matchPairsMany).
    std::vector<std::vector<Match>> matchPairsManyFloat( const std::vector<FeaturesDev*>& others, const MatchOptions& opts = MatchOptions() );
    /// matchPairsGuided against many objects in ONE device call (psx_match_pairs_guided_many_u8: one synchronisation, a
    /// number of launches that does not grow with others.size()), others[k] under guides[k]: element k equals
    /// matchPairsGuided( others[k], guides[k], opts ) with opts.bytes.  A guide of kind MatchGuide::None
    /// (MatchGuide::none()) skips its set: element k is empty.  Byte descriptors only.  Throws as matchPairsMany, for
    /// guides.size() != others.size(), and for a guide that is neither valid nor of kind None.
    std::vector<std::vector<Match>> matchPairsGuidedMany( const std::vector<FeaturesDev*>& others, const std::vector<MatchGuide>& guides,
                                                          const MatchOptions& opts );
    /// geometric verification: a homography (this = left -> other = right) estimated from `matches` (what matchPairs
    /// returned for the same two objects) by RANSAC on the device, psx_ransac_homography.  Throws as matchPairs, and for
    /// invalid options or a descriptor index outside its object.
    HomographyEstimate estimateHomography( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts = RansacOptions() );
    /// the same for a scene with depth: a fundamental matrix from at least 8 matches, psx_ransac_fundamental; its guide
    /// restricts matchPairsGuided to the epipolar band
    FundamentalEstimate estimateFundamental( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts = RansacOptions() );
    /// the registration models below a homography, for a scene that is one (video stabilisation, mosaics, a tracker's
    /// re-initialisation) or a match list too short for four points: a 2-D affine transform from at least 3 matches
    /// (psx_ransac_affine) and a similarity -- rotation, uniform scale, translation, no reflection -- from at least 2
    /// (psx_ransac_similarity).  The guide is a Homography whose last row is exactly (0, 0, 1)
    HomographyEstimate estimateAffine( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts = RansacOptions() );
    HomographyEstimate estimateSimilarity( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts = RansacOptions() );
    /// estimateHomography against many objects in ONE device call (psx_ransac_homography_many: one or two
    /// synchronisations and a number of launches that does not grow with others.size()): `matches` is what
    /// matchPairsMany( others ) returned, element k equals estimateHomography( others[k], matches[k], opts ).  Throws as
    /// estimateHomography, and when others and matches differ in size.
    /// From the result vector to the guides of matchPairsGuidedMany: guides[k] = est[k].best < 0 ? MatchGuide::none()
    /// : est[k].guide.  An estimate without a model carries a ZERO matrix, which as an Epipolar guide would admit every
    /// pair: it must become MatchGuide::none(), not be forwarded.
    std::vector<HomographyEstimate> estimateHomographyMany( const std::vector<FeaturesDev*>& others, const std::vector<std::vector<Match>>& matches,
                                                            const RansacOptions& opts = RansacOptions() );
    /// the same for fundamental matrices (psx_ransac_fundamental_many)
    std::vector<FundamentalEstimate> estimateFundamentalMany( const std::vector<FeaturesDev*>& others, const std::vector<std::vector<Match>>& matches,
                                                              const RansacOptions& opts = RansacOptions() );
    /// the same for affine transforms and similarities (psx_ransac_affine_many, psx_ransac_similarity_many)
    std::vector<HomographyEstimate> estimateAffineMany( const std::vector<FeaturesDev*>& others, const std::vector<std::vector<Match>>& matches,
                                                        const RansacOptions& opts = RansacOptions() );
    std::vector<HomographyEstimate> estimateSimilarityMany( const std::vector<FeaturesDev*>& others, const std::vector<std::vector<Match>>& matches,
                                                            const RansacOptions& opts = RansacOptions() );
    /// estimateHomography over a LIST OF VIEW PAIRS in ONE device call (psx_ransac_homography_graph: one or two
    /// synchronisations and a number of launches that grows neither with edges.size() nor with views.size()): `views`,
    /// `edges` and `matches` are what matchPairsGraph took and returned, element e equals
    /// views[left]->estimateHomography( views[right], matches[e], opts ) field by field, whatever the order of the list.
    /// Throws as estimateHomographyMany, for an edge index outside `views`, and when edges and matches differ in size.
    /// From the result vector to the guides of matchPairsGuidedGraph: as for estimateHomographyMany.
    static std::vector<HomographyEstimate> estimateHomographyGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                    const std::vector<std::vector<Match>>& matches,
                                                                    const RansacOptions& opts = RansacOptions() );
    /// the same for fundamental matrices, affine transforms and similarities (psx_ransac_fundamental_graph, _affine_graph,
    /// _similarity_graph)
    static std::vector<FundamentalEstimate> estimateFundamentalGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                      const std::vector<std::vector<Match>>& matches,
                                                                      const RansacOptions& opts = RansacOptions() );
    static std::vector<HomographyEstimate> estimateAffineGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                const std::vector<std::vector<Match>>& matches,
                                                                const RansacOptions& opts = RansacOptions() );
    static std::vector<HomographyEstimate> estimateSimilarityGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                    const std::vector<std::vector<Match>>& matches,
                                                                    const RansacOptions& opts = RansacOptions() );
    /// matchPairsGuided over a LIST OF VIEW PAIRS in ONE device call (psx_match_pairs_guided_graph_u8: one synchronisation,
    /// a number of launches that grows neither with edges.size() nor with views.size()), edge e under guides[e]: element
    /// e equals views[left]->matchPairsGuided( views[right], guides[e], opts ) with opts.bytes.  A guide of kind
    /// MatchGuide::None skips its edge: element e is empty.  Byte descriptors only.  Throws as matchPairsGraph, for
    /// guides.size() != edges.size(), and for a guide that is neither valid nor of kind None.
    static std::vector<std::vector<Match>> matchPairsGuidedGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                  const std::vector<MatchGuide>& guides, const MatchOptions& opts );
    /// matchPairsGraph on the views' FLOAT descriptors (psx_match_pairs_graph): no quantisation, no copies; element e equals
    /// views[left]->matchPairs( views[right], opts ) field by field, and estimate*Graph, matchPairsGuidedGraphFloat and
    /// tracks accept the lists unchanged.  Throws as matchPairsGraph for a null referenced entry, views on different devices
    /// and an edge index outside `views`, and for opts.bytes == true (use matchPairsGraph).
    static std::vector<std::vector<Match>> matchPairsGraphFloat( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                 const MatchOptions& opts = MatchOptions() );
    /// matchPairsGuidedMany on the objects' FLOAT descriptors (psx_match_pairs_guided_many): element k equals
    /// matchPairsGuided( others[k], guides[k], opts ) field by field; a guide of kind MatchGuide::None skips its set.
    /// Throws as matchPairsGuidedMany (a null entry, another device, one guide per object, an invalid guide), and for
    /// opts.bytes == true.
    std::vector<std::vector<Match>> matchPairsGuidedManyFloat( const std::vector<FeaturesDev*>& others, const std::vector<MatchGuide>& guides,
                                                               const MatchOptions& opts = MatchOptions() );
    /// matchPairsGuidedGraph on the views' FLOAT descriptors (psx_match_pairs_guided_graph): element e equals
    /// views[left]->matchPairsGuided( views[right], guides[e], opts ) field by field; a guide of kind MatchGuide::None skips
    /// its edge.  Throws as matchPairsGuidedGraph, and for opts.bytes == true.
    static std::vector<std::vector<Match>> matchPairsGuidedGraphFloat( const std::vector<FeaturesDev*>& views,
                                                                       const std::vector<std::pair<int,int>>& edges,
                                                                       const std::vector<MatchGuide>& guides, const MatchOptions& opts = MatchOptions() );

    /// The TRACKS of a list of view pairs in ONE device call (psx_tracks_graph: one synchronisation, a number of launches
    /// that grows neither with edges.size() nor with views.size()): the sets of descriptor rows in different views that
    /// `matches` connect transitively.  `views` and `edges` are what matchPairsGraph took, `matches` what matchPairsGraph,
    /// matchPairsGuidedGraph or -- as the inliers of their estimates -- estimate*Graph returned.  Tracks are over
    /// descriptor rows, as the matches are: the several orientations of one keypoint are not merged.  Throws as
    /// matchPairsGraph (a null referenced entry, views on different devices, an edge index outside `views`), when edges and
    /// matches differ in size, for min_views < 2, and for a match whose descriptor index lies outside its own edge's views.
    static Tracks buildTracks( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                               const std::vector<std::vector<Match>>& matches, const TrackOptions& opts = TrackOptions() );

    inline Feature*   getFeatures()    { return _ext; }
    inline Descriptor* getDescriptors() { return _ori; }
    inline int*        getReverseMap()  { return _rev; }
    inline void        setDevice( int d ) { _device = d; }
    inline int         getDevice() const  { return _device; }
};

} // namespace popsift
