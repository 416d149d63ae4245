// String helpers (reference: qmf/utils/Util.h:24-27).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace qmf {

// splits `str` on `delim`; an empty string gives no pieces, "a," gives {"a", ""}
std::vector<std::string> split(const std::string& str, const char delim);

// Addition: one int64 id per line (blank lines skipped); a line that is not a number, or a
// file that cannot be opened, aborts through CHECK
std::vector<int64_t> readIds(const std::string& fileName);

}  // namespace qmf
