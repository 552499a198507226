// meme_db -- reader of a MEME-format motif database, the other side of --compare.  CPU only, no
// device library behind it (host/tests/meme_db_dump.cpp prints what it read).
//
// What is read: a line `MOTIF id [alt]` starts a motif; its `letter-probability matrix:` line must carry `w= N` (any other
// token on it is ignored, so the files this program writes -- the MEME output, --refine's -- parse as well as the public
// collections); N rows of four numbers follow.  CRLF line ends and blank lines are tolerated, every other line is ignored
// (version, alphabet, strands, background, URL).  Rows need not be normalised: pengk_compare_quantize divides by their sum.
#ifndef PENGK_HOST_MEME_DB_H_
#define PENGK_HOST_MEME_DB_H_

#include <string>
#include <vector>

struct MemeMotif {
  std::string id, alt;
  int w = 0;
  std::vector<double> rows;  // w x 4, as written
};

// false, with *err naming the file, the line and the reason: the file cannot be read; a matrix line without a motif or
// without w=; w outside 1..max_w; a row that is not four numbers; a negative or non-finite entry; a row of zeros; a motif
// without a matrix; a file without a motif.
bool read_meme_db(const std::string& path, int max_w, std::vector<MemeMotif>* out, std::string* err);

#endif
