// FastaStream.h -- a FASTA file read block by block, for a streamed search (Havac::searchFastaFile).
//
// Across all blocks the reader yields exactly the characters FastaVector (FastaVector.h) holds for the whole file -- every
// record's residues with blanks and carriage returns dropped, a '\0' behind each record -- and the same record ends
// (sequenceEndPosition: one past the terminator, in columns of the whole text).  It runs the same line state machine as
// fastaVectorReadFasta over a buffer of kReadBuffer bytes of the file; headers are skipped, not kept.  It holds one block of
// text at a time.
#ifndef HAVAC_FASTA_STREAM_H
#define HAVAC_FASTA_STREAM_H

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

class FastaStreamReader {
public:
    static const size_t kReadBuffer = 1 << 20;
    explicit FastaStreamReader(const std::string &path);   // std::runtime_error when the file cannot be opened
    ~FastaStreamReader();
    FastaStreamReader(const FastaStreamReader &) = delete;
    FastaStreamReader &operator=(const FastaStreamReader &) = delete;

    // The next block: up to `maxChars` characters (fewer only at the end of the file).  text() / recordEnds() then hold the
    // block's characters and the ends of the records that end inside it.  Returns the characters read; 0 at the end.
    uint64_t readChars(uint64_t maxChars);
    // The next block of whole records: at least `minChars` characters, ending at a record's end -- a block grows to hold a
    // record longer than that (fewer only at the end of the file).
    uint64_t readRecords(uint64_t minChars);

    const std::vector<char> &text() const { return text_; }
    const std::vector<uint64_t> &recordEnds() const { return ends_; }
    uint64_t firstColumn() const { return first_; }      // the block's first character, in columns of the whole text
    uint64_t columns() const { return columns_; }        // characters read so far, all blocks
    uint64_t records() const { return records_; }        // records ended so far
    bool atEnd() const { return eof_ && pos_ == len_; }  // the file is read to its end
    uint64_t peakTextBytes() const { return peak_; }     // the most text one block has held

    // The columns of the block that are not a/c/g/t and their symbols, by SequencePreprocessor::collectPatches' rule, appended
    // (global columns); call once per block, in file order, so that rand() is drawn as for the whole file.
    void collectPatches(std::vector<uint64_t> &columns, std::vector<uint8_t> &symbols) const;

private:
    // appends to text_ until it holds `limit` characters, or a record has ended (stopAtRecordEnd), or the file has
    void fill(uint64_t limit, bool stopAtRecordEnd);
    void emit(char c) { text_.push_back(c); }
    void endRecord();
    std::FILE *f_ = nullptr;
    std::vector<char> buf_;
    size_t pos_ = 0, len_ = 0;
    bool eof_ = false, inRecord_ = false, inHeader_ = false, lineStart_ = true;
    std::vector<char> text_;
    std::vector<uint64_t> ends_;
    uint64_t first_ = 0, columns_ = 0, records_ = 0, peak_ = 0;
};
#endif
