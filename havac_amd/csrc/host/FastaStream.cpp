// FastaStream.cpp -- see FastaStream.h.  The state machine is fastaVectorReadFasta's (FastaVector.cpp), one block at a time.
#include "FastaStream.h"

#include <cstring>
#include <stdexcept>

#include "SequencePreprocessor.hpp"

FastaStreamReader::FastaStreamReader(const std::string &path) : buf_(kReadBuffer) {
    f_ = std::fopen(path.c_str(), "rb");
    if (!f_) throw std::runtime_error("Could not open fasta file for reading.");
}

FastaStreamReader::~FastaStreamReader() {
    if (f_) std::fclose(f_);
}

void FastaStreamReader::endRecord() {
    emit('\0');
    inRecord_ = false;
    records_++;
    ends_.push_back(first_ + text_.size());
}

static bool blank(char c) { return c == '\r' || c == ' ' || c == '\t'; }

void FastaStreamReader::fill(uint64_t limit, bool stopAtRecordEnd) {
    while (text_.size() < limit) {
        if (pos_ == len_) {
            if (eof_) return;
            len_ = std::fread(buf_.data(), 1, buf_.size(), f_);
            pos_ = 0;
            if (len_ == 0) {
                if (std::ferror(f_)) throw std::runtime_error("Error while reading from the opened fasta file.");
                eof_ = true;
                inHeader_ = false;
                if (inRecord_) endRecord();
                return;
            }
            continue;
        }
        const char *const buf = buf_.data();
        const char *nl = static_cast<const char *>(std::memchr(buf + pos_, '\n', len_ - pos_));
        const size_t end = nl ? (size_t)(nl - buf) : len_;        // segment [pos_, end), newline (if any) at end
        if (inHeader_) {                                           // headers are not kept
            if (nl) { inHeader_ = false; lineStart_ = true; }
            pos_ = nl ? end + 1 : len_;
            continue;
        }
        if (pos_ == end) {                                         // an empty line
            lineStart_ = true;
            pos_ = end + 1;
            continue;
        }
        if (lineStart_ && buf[pos_] == '>') {
            const bool ended = inRecord_;
            if (ended) endRecord();
            inRecord_ = inHeader_ = true;                          // (the record of this header)
            lineStart_ = false;
            pos_++;
            if (ended && stopAtRecordEnd) return;
            continue;
        }
        lineStart_ = false;
        if (!inRecord_) {                                          // residues before any header: an unnamed record
            for (size_t r = pos_; r < end && !inRecord_; r++) inRecord_ = !blank(buf[r]);
        }
        if (inRecord_) {
            // residues, as many as the block has room for; blanks are dropped
            const uint64_t room = limit - text_.size();
            size_t take = (size_t)std::min<uint64_t>(room, end - pos_);
            if (!std::memchr(buf + pos_, '\r', take) && !std::memchr(buf + pos_, ' ', take) && !std::memchr(buf + pos_, '\t', take)) {
                text_.insert(text_.end(), buf + pos_, buf + pos_ + take);
                pos_ += take;
            } else {
                size_t r = pos_;
                for (; r < end && text_.size() < limit; r++)
                    if (!blank(buf[r])) emit(buf[r]);
                while (r < end && blank(buf[r])) r++;              // (trailing blanks belong to no block)
                pos_ = r;
            }
            if (pos_ < end) return;                                // the block is full
        } else {
            pos_ = end;
        }
        if (nl) { lineStart_ = true; pos_ = end + 1; }
    }
}

uint64_t FastaStreamReader::readChars(uint64_t maxChars) {
    first_ += text_.size();
    text_.clear();
    ends_.clear();
    if (text_.capacity() < maxChars && maxChars <= (1ull << 34)) text_.reserve(maxChars);
    fill(maxChars, false);
    columns_ += text_.size();
    peak_ = std::max<uint64_t>(peak_, text_.size());
    return text_.size();
}

uint64_t FastaStreamReader::readRecords(uint64_t minChars) {
    first_ += text_.size();
    text_.clear();
    ends_.clear();
    if (text_.capacity() < minChars && minChars <= (1ull << 34)) text_.reserve(minChars);
    fill(minChars, false);
    // finish the record the block stopped in
    auto atRecordEnd = [&] { return !ends_.empty() && ends_.back() == first_ + text_.size(); };
    while (!text_.empty() && !atRecordEnd()) {
        const size_t before = text_.size();
        fill(before + kReadBuffer, true);
        if (text_.size() == before) break;                         // (the file ended inside no record)
    }
    columns_ += text_.size();
    peak_ = std::max<uint64_t>(peak_, text_.size());
    return text_.size();
}

void FastaStreamReader::collectPatches(std::vector<uint64_t> &columns, std::vector<uint8_t> &symbols) const {
    SequencePreprocessor::collectPatches(text_.data(), text_.size(), first_, atEnd(), columns, symbols);
}
