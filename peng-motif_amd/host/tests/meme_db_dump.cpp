// meme_db_dump FILE -- prints what read_meme_db makes of a motif database: per motif a line `MOTIF id alt|- w`, then its
// rows as written (%.17g).  Exit code 4 and the reader's message on stderr for a file it rejects (as peng_motif
// --compare-db).  CPU only; tests/test_motif_compare_cpu.py.
#include <cstdio>

#include "meme_db.h"

int main(int nargs, char** args) {
  if (nargs != 2) {
    fprintf(stderr, "usage: meme_db_dump FILE\n");
    return 2;
  }
  std::vector<MemeMotif> db;
  std::string err;
  if (!read_meme_db(args[1], 64, &db, &err)) {
    fprintf(stderr, "ERROR: %s\n", err.c_str());
    return 4;
  }
  for (const MemeMotif& m : db) {
    printf("MOTIF %s %s %d\n", m.id.c_str(), m.alt.empty() ? "-" : m.alt.c_str(), m.w);
    for (int j = 0; j < m.w; ++j)
      printf("%.17g %.17g %.17g %.17g\n", m.rows[4 * j], m.rows[4 * j + 1], m.rows[4 * j + 2], m.rows[4 * j + 3]);
  }
  return 0;
}
