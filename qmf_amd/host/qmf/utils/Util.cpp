#include <qmf/utils/Util.h>

#include <charconv>
#include <fstream>

#include <qmf/utils/Log.h>

namespace qmf {

std::vector<std::string> split(const std::string& str, const char delim) {
  std::vector<std::string> out;
  if (str.empty()) return out;
  size_t start = 0;
  for (;;) {
    const size_t end = str.find(delim, start);
    out.emplace_back(str, start, end == std::string::npos ? std::string::npos : end - start);
    if (end == std::string::npos) break;
    start = end + 1;
  }
  return out;
}

std::vector<int64_t> readIds(const std::string& fileName) {
  std::ifstream in(fileName);
  CHECK(in.good()) << "cannot open " << fileName;
  std::vector<int64_t> ids;
  std::string line;
  while (std::getline(in, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    int64_t id = 0;
    const auto r = std::from_chars(line.data(), line.data() + line.size(), id);
    CHECK(r.ec == std::errc() && r.ptr == line.data() + line.size())
        << "the file format is incorrect: " << line;
    ids.push_back(id);
  }
  return ids;
}

}  // namespace qmf
