#include "meme_db.h"

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <sstream>

namespace {
std::vector<std::string> tokens(const std::string& line) {
  std::vector<std::string> t;
  std::istringstream in(line);
  std::string s;
  while (in >> s) t.push_back(s);  // (a trailing \r is white space to >>)
  return t;
}

bool number(const std::string& s, double* v) {
  char* end = nullptr;
  *v = std::strtod(s.c_str(), &end);
  return end != s.c_str() && *end == 0;
}
}  // namespace

bool read_meme_db(const std::string& path, int max_w, std::vector<MemeMotif>* out, std::string* err) {
  out->clear();
  std::ifstream in(path, std::ios::binary);
  size_t line_no = 0;
  auto bad = [&](const std::string& why) {
    std::ostringstream o;
    o << "motif database " << path;
    if (line_no) o << ", line " << line_no;
    o << ": " << why;
    *err = o.str();
    return false;
  };
  if (!in.is_open()) return bad("cannot be opened");
  std::string line;
  bool have_motif = false, have_matrix = true;  // (of the motif that is open)
  int rows_left = 0;
  while (std::getline(in, line)) {
    ++line_no;
    const std::vector<std::string> t = tokens(line);
    if (t.empty()) continue;
    if (rows_left) {
      MemeMotif& m = out->back();
      if (t.size() != 4) return bad("motif " + m.id + ": a matrix row must hold four numbers");
      double v[4], sum = 0.0;
      for (int a = 0; a < 4; ++a) {
        if (!number(t[a], &v[a]) || !std::isfinite(v[a])) return bad("motif " + m.id + ": '" + t[a] + "' is not a number");
        if (v[a] < 0.0) return bad("motif " + m.id + ": negative entry " + t[a]);
        sum += v[a];
      }
      if (!(sum > 0.0)) return bad("motif " + m.id + ": a row of zeros");
      m.rows.insert(m.rows.end(), v, v + 4);
      --rows_left;
      continue;
    }
    if (t[0] == "MOTIF") {
      if (have_motif && !have_matrix) return bad("motif " + out->back().id + " has no letter-probability matrix");
      if (t.size() < 2) return bad("MOTIF without an identifier");
      out->emplace_back();
      out->back().id = t[1];
      if (t.size() > 2) out->back().alt = t[2];
      have_motif = true;
      have_matrix = false;
    } else if (t[0] == "letter-probability" && t.size() > 1 && t[1] == "matrix:") {
      if (!have_motif || have_matrix) return bad("a letter-probability matrix without a MOTIF line");
      long w = -1;
      bool found = false;
      for (size_t i = 2; i < t.size() && !found; ++i) {
        std::string val;
        if (t[i] == "w=" && i + 1 < t.size()) val = t[i + 1];
        else if (t[i].size() > 2 && t[i].compare(0, 2, "w=") == 0) val = t[i].substr(2);
        else continue;
        char* end = nullptr;
        w = std::strtol(val.c_str(), &end, 10);
        if (end == val.c_str() || *end) return bad("motif " + out->back().id + ": w= '" + val + "' is not an integer");
        found = true;
      }
      if (!found) return bad("motif " + out->back().id + ": the matrix line carries no w=");
      if (w < 1 || w > max_w) {
        std::ostringstream o;
        o << "motif " << out->back().id << ": w= " << w << " outside 1.." << max_w;
        return bad(o.str());
      }
      out->back().w = (int)w;
      rows_left = (int)w;
      have_matrix = true;
    }
  }
  if (rows_left) return bad("motif " + out->back().id + ": the file ends inside its matrix (a matrix row must hold four numbers)");
  if (have_motif && !have_matrix) return bad("motif " + out->back().id + " has no letter-probability matrix");
  line_no = 0;
  if (out->empty()) return bad("no motif in the file");
  return true;
}
