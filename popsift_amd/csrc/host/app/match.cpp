// popsift-match -- MatchingMode tool with the reference's option surface (src/application/match.cpp:49-300):
// extracts two images into FeaturesDev objects and prints one accept / reject line per left descriptor
// (FeaturesDev::match, features.cu:227-304).  Not in the reference tool: --pairs FILE writes the matches as data
// (FeaturesDev::matchPairs) instead of the accept / reject lines; --ratio and --mutual refine it; --homography or
// --fundamental with --guide-tol restrict the search to the pairs a guide admits (FeaturesDev::matchPairsGuided);
// --verify-homography TOL estimates a homography from the pairs (FeaturesDev::estimateHomography) and writes its inliers,
// --verify-fundamental TOL a fundamental matrix (FeaturesDev::estimateFundamental), --verify-affine TOL a 2-D affine
// transform (estimateAffine), --verify-similarity TOL a similarity (estimateSimilarity); --rematch then writes the list
// guided by that model instead.
#include "options.h"
#include "pgmread.h"

#include <popsift/common/device_prop.h>
#include <popsift/features.h>
#include <popsift/popsift.h>
#include <popsift/sift_conf.h>
#include <popsift/version.hpp>

#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

using namespace std;

static bool print_dev_info = false;
static bool uchar_desc = false;
static string pairs_file;
static bool  have_ratio = false, mutual = false;
static float pair_ratio = 0.8f;
static bool  have_h = false, have_f = false, have_tol = false;
static popsift::MatchGuide guide;
static bool  have_verify = false, have_ransac_opt = false, rematch = false;
// the models of --verify-*: option name, the name printed, the model in an error message
enum { VerifyHomography, VerifyFundamental, VerifyAffine, VerifySimilarity, VerifyModels };
static const char* const verify_names[VerifyModels][3] = { { "verify-homography", "Homography", "homography" },
                                                            { "verify-fundamental", "Fundamental", "fundamental matrix" },
                                                            { "verify-affine", "Affine", "affine transform" },
                                                            { "verify-similarity", "Similarity", "similarity" } };
static const char* const verify_list = "'--verify-homography', '--verify-fundamental', '--verify-affine' or '--verify-similarity'";
static bool  verify_given[VerifyModels] = { false, false, false, false };
static popsift::RansacOptions ransac;

// "m0,...,m8": nine numbers, row major
static void parse_matrix( const string& opt, const string& s, float* m )
{
    size_t pos = 0;
    for( int k = 0; k < 9; k++ ) {
        const size_t end = k < 8 ? s.find( ',', pos ) : s.size();
        if( end == string::npos ) throw runtime_error( "the option '--" + opt + "' takes nine numbers m0,...,m8" );
        const string v = s.substr( pos, end - pos );
        try { m[k] = app::to_float( v ); }
        catch( const std::logic_error& ) { throw runtime_error( "bad number '" + v + "' in the option '--" + opt + "'" ); }
        pos = end + 1;
    }
}

static bool is_file( const string& p ) { struct stat st; return stat( p.c_str(), &st ) == 0 && S_ISREG( st.st_mode ); }

static SiftJob* process_image( const string& inputFile, PopSift& sift )
{
    int w = 0, h = 0;
    unsigned char* image_data = readPGMfile( inputFile, w, h );
    if( image_data == nullptr ) exit( EXIT_FAILURE );
    cout << "Loading " << w << " x " << h << " image " << inputFile << endl;
    SiftJob* job = sift.enqueue( w, h, image_data );
    delete[] image_data;
    return job;
}

int main( int argc, char** argv )
{
    popsift::Config config;
    string lFile, rFile;
    cout << "PopSift version: " << POPSIFT_VERSION_STRING << endl;

    ransac.refit = false;                   // the tool refits on request (--ransac-refit)
    app::Options all;
    bool help = false;
    all.flag( "help", 'h', "Print usage", [&]() { help = true; } );
    all.flag( "verbose", 'v', "", [&]() { config.setVerbose(); } );
    all.flag( "log", 0, "Write debugging files", [&]() { config.setLogMode( popsift::Config::All ); } );
    all.add( "left", 'l', true, "\"Left\"  input file", [&]( const string& s ) { lFile = s; } );
    all.add( "right", 'r', true, "\"Right\" input file", [&]( const string& s ) { rFile = s; } );
    app::add_config_options( all, config );
    all.flag( "print-dev-info", 0, "A debug output printing device information", [&]() { print_dev_info = true; } );
    all.flag( "print-time-info", 0, "accepted for compatibility", []() {} );
    all.flag( "write-as-uchar", 0, "accepted for compatibility", []() {} );
    all.flag( "dont-write", 0, "accepted for compatibility", []() {} );
    // not in the reference tool: quantise both descriptor sets to bytes and run the exact integer matcher
    all.flag( "uchar-descriptors", 0, "Match byte descriptors (FeaturesDev::matchBytes)", [&]() { uchar_desc = true; } );
    all.add( "pairs", 0, true, "Write the matches to this file, one line per pair: left_feature left_descriptor right_feature "
             "right_descriptor distance second_distance (instead of the accept / reject lines)", [&]( const string& s ) { pairs_file = s; } );
    all.add( "ratio", 0, true, "Keep a pair iff distance / second_distance < ratio; 'inf' switches the test off. Default is 0.8 (needs --pairs)",
             [&]( const string& s ) { pair_ratio = app::to_float( s ); have_ratio = true; } );
    all.flag( "mutual", 0, "Keep a pair only if each descriptor is the other's nearest neighbour (needs --pairs)", [&]() { mutual = true; } );
    all.add( "homography", 0, true, "Guided matching: m0,...,m8 = H, row major; keep a right point only within --guide-tol pixels of "
             "H * left point (needs --pairs and --guide-tol)", [&]( const string& s ) { parse_matrix( "homography", s, guide.m ); have_h = true; } );
    all.add( "fundamental", 0, true, "Guided matching: m0,...,m8 = F, row major; keep a right point only within --guide-tol pixels of "
             "the line F * left point (needs --pairs and --guide-tol)", [&]( const string& s ) { parse_matrix( "fundamental", s, guide.m ); have_f = true; } );
    all.add( "guide-tol", 0, true, "Guided matching: the tolerance in pixels (needs --homography or --fundamental)",
             [&]( const string& s ) { guide.tol = app::to_float( s ); have_tol = true; } );
    all.add( "verify-homography", 0, true, "Geometric verification: estimate a homography from the pairs by RANSAC with this inlier "
             "tolerance in pixels, print it and write only its inliers (needs --pairs)",
             [&]( const string& s ) { ransac.tol = app::to_float( s ); verify_given[VerifyHomography] = true; } );
    all.add( "verify-fundamental", 0, true, "Geometric verification: estimate a fundamental matrix from the pairs by RANSAC with this "
             "inlier tolerance in pixels (distance from the epipolar line), print it and write only its inliers (needs --pairs)",
             [&]( const string& s ) { ransac.tol = app::to_float( s ); verify_given[VerifyFundamental] = true; } );
    all.add( "verify-affine", 0, true, "Geometric verification: estimate a 2-D affine transform (3-point samples) from the pairs by RANSAC "
             "with this inlier tolerance in pixels, print it and write only its inliers (needs --pairs)",
             [&]( const string& s ) { ransac.tol = app::to_float( s ); verify_given[VerifyAffine] = true; } );
    all.add( "verify-similarity", 0, true, "Geometric verification: estimate a similarity -- rotation, uniform scale, translation; 2-point "
             "samples -- from the pairs by RANSAC with this inlier tolerance in pixels, print it and write only its inliers (needs --pairs)",
             [&]( const string& s ) { ransac.tol = app::to_float( s ); verify_given[VerifySimilarity] = true; } );
    all.add( "ransac-hypotheses", 0, true, "Geometric verification: the number of hypotheses, 1 to 65536. Default is 1024",
             [&]( const string& s ) { ransac.hypotheses = (int)app::to_float( s ); have_ransac_opt = true; } );
    all.add( "ransac-seed", 0, true, "Geometric verification: the seed of the samples. Default is 0",
             [&]( const string& s ) { ransac.seed = (unsigned)std::strtoul( s.c_str(), nullptr, 10 ); have_ransac_opt = true; } );
    all.flag( "ransac-refit", 0, "Geometric verification: refit the best hypothesis over its inliers", [&]() { ransac.refit = true; have_ransac_opt = true; } );
    all.flag( "rematch", 0, "After --verify-homography, --verify-fundamental, --verify-affine or --verify-similarity: match again, guided by the estimated model and the "
              "same tolerance, and write that list instead", [&]() { rematch = true; } );
    all.flag( "pgmread-loading", 0, "Use the PGM/PPM loader (the only loader of this build)", []() {} );
    int verify_model = VerifyHomography;
    try {
        all.parse( argc, argv );
        if( help ) { all.usage( cout ); return EXIT_SUCCESS; }
        if( lFile.empty() || rFile.empty() ) throw runtime_error( "the options '--left' and '--right' are required" );
        if( ( have_ratio || mutual ) && pairs_file.empty() ) throw runtime_error( "the options '--ratio' and '--mutual' need '--pairs'" );
        if( have_ratio && !( pair_ratio > 0.0f ) ) throw runtime_error( "the ratio must be positive" );
        if( have_h && have_f ) throw runtime_error( "at most one of the options '--homography' and '--fundamental' may be given" );
        if( ( have_h || have_f ) && pairs_file.empty() ) throw runtime_error( "the options '--homography' and '--fundamental' need '--pairs'" );
        if( have_tol && !( have_h || have_f ) ) throw runtime_error( "the option '--guide-tol' needs '--homography' or '--fundamental'" );
        if( ( have_h || have_f ) && !have_tol ) throw runtime_error( "the options '--homography' and '--fundamental' need '--guide-tol'" );
        if( have_tol && !( guide.tol >= 0.0f && std::isfinite( guide.tol ) ) ) throw runtime_error( "the guide tolerance must be finite and not negative" );
        guide.kind = have_f ? popsift::MatchGuide::Epipolar : popsift::MatchGuide::Homography;
        for( int k = 0; k < VerifyModels; k++ ) {
            if( !verify_given[k] ) continue;
            if( have_verify ) throw runtime_error( string( "the options '--" ) + verify_names[verify_model][0] + "' and '--" + verify_names[k][0] + "' cannot be combined" );
            have_verify = true; verify_model = k;
        }
        const string verify_opt = string( "'--" ) + verify_names[verify_model][0] + "'";
        if( have_verify && pairs_file.empty() ) throw runtime_error( "the option " + verify_opt + " needs '--pairs'" );
        if( have_ransac_opt && !have_verify ) throw runtime_error( string( "the options '--ransac-hypotheses', '--ransac-seed' and '--ransac-refit' need " ) + verify_list );
        if( rematch && !have_verify ) throw runtime_error( string( "the option '--rematch' needs " ) + verify_list );
        if( have_verify && ( have_h || have_f ) ) throw runtime_error( "the option " + verify_opt + " cannot be combined with '--homography' or '--fundamental'" );
        if( have_verify && !( ransac.tol >= 0.0f && std::isfinite( ransac.tol ) ) ) throw runtime_error( "the verification tolerance must be finite and not negative" );
        if( have_verify && ( ransac.hypotheses < 1 || ransac.hypotheses > 65536 ) ) throw runtime_error( "the number of hypotheses must lie in 1 .. 65536" );
    } catch( const std::exception& e ) {
        cerr << "Error: " << e.what() << endl << endl << "Usage:" << endl << endl;
        all.usage( cerr );
        return EXIT_FAILURE;
    }
    cout << lFile << " <-> " << rFile << endl;
    for( const string& f : { lFile, rFile } )
        if( !is_file( f ) ) { cout << "Input file " << f << " is not a regular file, nothing to do" << endl; return EXIT_FAILURE; }

    popsift::cuda::device_prop_t deviceInfo;
    deviceInfo.set( 0, print_dev_info );
    if( print_dev_info ) deviceInfo.print();

    try {
        PopSift sift( config, popsift::Config::MatchingMode );
        SiftJob* lJob = process_image( lFile, sift );
        SiftJob* rJob = process_image( rFile, sift );
        popsift::FeaturesDev* lFeatures = lJob->getDev();
        cout << "Number of features:    " << lFeatures->getFeatureCount() << endl;
        cout << "Number of descriptors: " << lFeatures->getDescriptorCount() << endl;
        popsift::FeaturesDev* rFeatures = rJob->getDev();
        cout << "Number of features:    " << rFeatures->getFeatureCount() << endl;
        cout << "Number of descriptors: " << rFeatures->getDescriptorCount() << endl;
        cout.flush();
        if( !pairs_file.empty() ) {
            popsift::MatchOptions mo;
            mo.ratio = pair_ratio; mo.mutual = mutual; mo.bytes = uchar_desc;
            std::vector<popsift::Match> mm = ( have_h || have_f ) ? lFeatures->matchPairsGuided( rFeatures, guide, mo )
                                                                  : lFeatures->matchPairs( rFeatures, mo );
            if( have_verify ) {
                const char* model = verify_names[verify_model][1];
                const popsift::HomographyEstimate est = verify_model == VerifyFundamental ? lFeatures->estimateFundamental( rFeatures, mm, ransac )
                                                      : verify_model == VerifyAffine      ? lFeatures->estimateAffine( rFeatures, mm, ransac )
                                                      : verify_model == VerifySimilarity  ? lFeatures->estimateSimilarity( rFeatures, mm, ransac )
                                                                                          : lFeatures->estimateHomography( rFeatures, mm, ransac );
                printf( "%s:", model );
                for( int k = 0; k < 9; k++ ) printf( " %.9g", est.guide.m[k] );
                printf( "\n%s inliers: %d of %d\n", model, (int)est.inliers.size(), (int)mm.size() );
                if( est.best < 0 ) throw runtime_error( string( "no " ) + verify_names[verify_model][2] + " could be estimated from the pairs" );
                mm = rematch ? lFeatures->matchPairsGuided( rFeatures, est.guide, mo ) : est.inliers;
            }
            FILE* f = fopen( pairs_file.c_str(), "w" );
            if( f == nullptr ) throw runtime_error( "cannot write " + pairs_file );
            for( const popsift::Match& m : mm )
                fprintf( f, "%d %d %d %d %.3f %.3f\n", m.left_feature, m.left_descriptor, m.right_feature, m.right_descriptor,
                         m.distance, m.second_distance );
            fclose( f );
            cout << "Number of matches: " << mm.size() << endl;
        }
        else if( uchar_desc ) lFeatures->matchBytes( rFeatures );
        else                  lFeatures->match( rFeatures );
        fflush( stdout );
        delete lFeatures; delete rFeatures; delete lJob; delete rJob;
        sift.uninit();
    } catch( const std::exception& e ) {
        cerr << e.what() << endl;
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
