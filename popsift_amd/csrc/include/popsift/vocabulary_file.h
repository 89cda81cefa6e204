/* The file a popsift::Vocabulary is kept in (popsift/shortlist.h: Vocabulary::save / load).  Plain C++11: no HIP, no call
 * into the library, so a stand-alone program can include this header alone (tests/cpp/query_san.cpp does).
 *
 * Little endian, whatever the host:
 *     bytes 0 .. 7     the magic "PSXVOCAB"
 *     uint32           version   (1)
 *     uint32           words     (2 .. 65536)
 *     uint32           dimension (128)
 *     words x 128      the words, one byte per component
 *     uint64           FNV-1a (64 bit) of every byte before it
 * Training is the one step of the shortlist a deployment does once and stores: a file of W = 4096 words is 512 KiB. */
#pragma once

#include <cstddef>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace popsift {
namespace vocabulary_file {

const char     MAGIC[9]  = "PSXVOCAB";
const unsigned VERSION   = 1;
const unsigned DIMENSION = 128;
const unsigned MIN_WORDS = 2;
const unsigned MAX_WORDS = 65536;
const size_t   HEAD      = 8 + 3 * 4;

inline unsigned long long fnv1a( const unsigned char* p, size_t n )
{
    unsigned long long h = 14695981039346656037ULL;
    for( size_t i = 0; i < n; i++ ) { h ^= p[i]; h *= 1099511628211ULL; }
    return h;
}

inline void put( std::vector<unsigned char>& out, unsigned long long v, int bytes )
{
    for( int b = 0; b < bytes; b++ ) out.push_back( (unsigned char)( v >> ( 8 * b ) ) );
}

inline unsigned long long get( const unsigned char* p, int bytes )
{
    unsigned long long v = 0;
    for( int b = 0; b < bytes; b++ ) v |= (unsigned long long)p[b] << ( 8 * b );
    return v;
}

/// the bytes of a file holding `words` words of 128 bytes
inline std::vector<unsigned char> encode( const unsigned char* bytes, unsigned words )
{
    if( bytes == nullptr || words < MIN_WORDS || words > MAX_WORDS ) throw std::runtime_error( "vocabulary file: words outside [2, 65536]" );
    std::vector<unsigned char> out;
    out.reserve( HEAD + (size_t)words * DIMENSION + 8 );
    out.insert( out.end(), MAGIC, MAGIC + 8 );
    put( out, VERSION, 4 );
    put( out, words, 4 );
    put( out, DIMENSION, 4 );
    out.insert( out.end(), bytes, bytes + (size_t)words * DIMENSION );
    put( out, fnv1a( out.data(), out.size() ), 8 );
    return out;
}

/// the words of a file's bytes; std::runtime_error for a short file, a wrong magic, version or dimension, words outside
/// [2, 65536], bytes behind the checksum, or a checksum that does not match
inline std::vector<unsigned char> decode( const unsigned char* file, size_t size )
{
    if( file == nullptr || size < HEAD ) throw std::runtime_error( "vocabulary file: too short for a header" );
    for( int i = 0; i < 8; i++ )
        if( file[i] != (unsigned char)MAGIC[i] ) throw std::runtime_error( "vocabulary file: wrong magic" );
    if( get( file + 8, 4 ) != VERSION ) throw std::runtime_error( "vocabulary file: unknown version" );
    const unsigned long long words = get( file + 12, 4 );
    if( words < MIN_WORDS || words > MAX_WORDS ) throw std::runtime_error( "vocabulary file: words outside [2, 65536]" );
    if( get( file + 16, 4 ) != DIMENSION ) throw std::runtime_error( "vocabulary file: dimension is not 128" );
    const size_t body = HEAD + (size_t)words * DIMENSION;
    if( size < body + 8 ) throw std::runtime_error( "vocabulary file: shorter than its header says" );
    if( size > body + 8 ) throw std::runtime_error( "vocabulary file: longer than its header says" );
    if( get( file + body, 8 ) != fnv1a( file, body ) ) throw std::runtime_error( "vocabulary file: checksum mismatch" );
    return std::vector<unsigned char>( file + HEAD, file + body );
}

inline void write( const std::string& path, const unsigned char* bytes, unsigned words )
{
    const std::vector<unsigned char> out = encode( bytes, words );
    std::FILE* f = std::fopen( path.c_str(), "wb" );
    if( f == nullptr ) throw std::runtime_error( "vocabulary file: cannot create " + path );
    const bool ok = std::fwrite( out.data(), 1, out.size(), f ) == out.size();
    if( std::fclose( f ) != 0 || !ok ) throw std::runtime_error( "vocabulary file: cannot write " + path );
}

inline std::vector<unsigned char> read( const std::string& path )
{
    std::FILE* f = std::fopen( path.c_str(), "rb" );
    if( f == nullptr ) throw std::runtime_error( "vocabulary file: cannot open " + path );
    // the largest valid file and one byte: a longer one is refused by its size, whatever it holds
    std::vector<unsigned char> in( HEAD + (size_t)MAX_WORDS * DIMENSION + 8 + 1 );
    const size_t n = std::fread( in.data(), 1, in.size(), f );
    const bool bad = std::ferror( f ) != 0;
    std::fclose( f );
    if( bad ) throw std::runtime_error( "vocabulary file: cannot read " + path );
    return decode( in.data(), n );
}

} // namespace vocabulary_file
} // namespace popsift
