// rip_yaml.cpp -- the YAML-subset reader (rip_yaml.hpp).
#include "rip_yaml.hpp"

#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <sstream>

namespace rip {

// =============================================================================================
// YAML subset
// =============================================================================================
namespace {
const YamlNode kNullNode;

std::string trim(const std::string& s) {
  size_t a = s.find_first_not_of(" \t\r\n");
  if (a == std::string::npos) return "";
  size_t b = s.find_last_not_of(" \t\r\n");
  return s.substr(a, b - a + 1);
}

std::string strip_comment(const std::string& line) {
  bool sq = false, dq = false;
  for (size_t i = 0; i < line.size(); i++) {
    char c = line[i];
    if (c == '\'' && !dq) sq = !sq;
    if (c == '"' && !sq) dq = !dq;
    if (c == '#' && !sq && !dq && (i == 0 || line[i - 1] == ' ' || line[i - 1] == '\t')) return line.substr(0, i);
  }
  return line;
}

std::string unquote(const std::string& s) {
  if (s.size() >= 2 && ((s.front() == '"' && s.back() == '"') || (s.front() == '\'' && s.back() == '\'')))
    return s.substr(1, s.size() - 2);
  return s;
}

struct Line {
  int indent;
  std::string text;
  int number;
};

std::vector<std::string> split_flow(const std::string& body, int line_no) {
  std::vector<std::string> out;
  std::string cur;
  for (char c : body) {
    if (c == ',') {
      out.push_back(unquote(trim(cur)));
      cur.clear();
    } else if (c == '[' || c == ']' || c == '{' || c == '}') {
      throw YamlError("yaml: nested flow collections are not supported (line " + std::to_string(line_no) + ")");
    } else {
      cur += c;
    }
  }
  if (!trim(cur).empty()) out.push_back(unquote(trim(cur)));
  return out;
}

// Nesting the reader follows (both parsers recurse once per level; a document nested deeper than any configuration file of
// the reference -- three levels -- by an order of magnitude is refused instead of overflowing the stack: tests/test_host_fuzz.py)
constexpr int kMaxYamlDepth = 64;

// flow map starting at text[at] == '{'; leaves `at` behind the closing brace
void parse_flow_map(const std::string& text, size_t& at, int line_no, YamlNode& node, int depth = 0) {
  auto fail = [&](const char* what) { throw YamlError(std::string("yaml: ") + what + " (line " + std::to_string(line_no) + ")"); };
  if (depth > kMaxYamlDepth) fail("flow maps nested too deeply");
  auto skip_ws = [&]() { while (at < text.size() && (text[at] == ' ' || text[at] == '\t')) at++; };
  node.kind = YamlNode::Map;
  at++;  // '{'
  for (;;) {
    skip_ws();
    if (at >= text.size()) fail("unterminated flow map");
    if (text[at] == '}') { at++; return; }
    size_t colon = text.find(':', at);
    if (colon == std::string::npos) fail("expected 'key: value' in flow map");
    const std::string key = unquote(trim(text.substr(at, colon - at)));
    if (key.empty() || key.find_first_of("{}[],") != std::string::npos) fail("bad key in flow map");
    at = colon + 1;
    skip_ws();
    YamlNode child;
    if (at < text.size() && text[at] == '{') {
      parse_flow_map(text, at, line_no, child, depth + 1);
    } else if (at < text.size() && text[at] == '[') {
      size_t close = text.find(']', at);
      if (close == std::string::npos) fail("unterminated '[' in flow map");
      child.kind = YamlNode::Sequence;
      child.seq = split_flow(text.substr(at + 1, close - at - 1), line_no);
      at = close + 1;
    } else {
      size_t end = text.find_first_of(",}", at);
      if (end == std::string::npos) fail("unterminated flow map");
      const std::string v = trim(text.substr(at, end - at));
      if (!v.empty()) {
        child.kind = YamlNode::Scalar;
        child.scalar = unquote(v);
      }
      at = end;
    }
    node.map[key] = child;
    skip_ws();
    if (at < text.size() && text[at] == ',') at++;
    else if (at >= text.size() || text[at] != '}') fail("expected ',' or '}' in flow map");
  }
}

// parses lines[pos..) with indentation == indent into `node` (a map)
void parse_block(const std::vector<Line>& lines, size_t& pos, int indent, YamlNode& node, int depth = 0) {
  node.kind = YamlNode::Map;
  if (depth > kMaxYamlDepth) throw YamlError("yaml: blocks nested too deeply at line " + std::to_string(pos < lines.size() ? lines[pos].number : 0));
  while (pos < lines.size()) {
    const Line& ln = lines[pos];
    if (ln.indent < indent) return;
    if (ln.indent > indent) throw YamlError("yaml: unexpected indentation at line " + std::to_string(ln.number));
    if (ln.text[0] == '-') throw YamlError("yaml: block sequences are not supported (line " + std::to_string(ln.number) + ")");
    size_t colon = std::string::npos;
    {
      bool sq = false, dq = false;
      for (size_t i = 0; i < ln.text.size(); i++) {
        char c = ln.text[i];
        if (c == '\'' && !dq) sq = !sq;
        if (c == '"' && !sq) dq = !dq;
        if (c == ':' && !sq && !dq && (i + 1 == ln.text.size() || ln.text[i + 1] == ' ')) {
          colon = i;
          break;
        }
      }
    }
    if (colon == std::string::npos) throw YamlError("yaml: expected 'key: value' at line " + std::to_string(ln.number));
    std::string key = unquote(trim(ln.text.substr(0, colon)));
    std::string val = trim(ln.text.substr(colon + 1));
    pos++;
    YamlNode child;
    if (val.empty()) {
      if (pos < lines.size() && lines[pos].indent > indent) {
        parse_block(lines, pos, lines[pos].indent, child, depth + 1);
      }  // else: null
    } else if (val[0] == '[') {
      std::string body = val.substr(1);
      int number = ln.number;
      while (body.find(']') == std::string::npos) {
        if (pos >= lines.size()) throw YamlError("yaml: unterminated '[' opened at line " + std::to_string(number));
        body += " " + lines[pos].text;
        pos++;
      }
      size_t close = body.find(']');
      if (!trim(body.substr(close + 1)).empty()) throw YamlError("yaml: trailing characters after ']' (line " + std::to_string(number) + ")");
      child.kind = YamlNode::Sequence;
      child.seq = split_flow(body.substr(0, close), number);
    } else if (val[0] == '{') {
      // flow map {key: value, key: [a, b], key: {...}}; may continue on the following lines
      std::string body = val;
      int number = ln.number;
      auto depth_of = [](const std::string& t) {
        int d = 0;
        for (char c : t) d += (c == '{' || c == '[') ? 1 : ((c == '}' || c == ']') ? -1 : 0);
        return d;
      };
      while (depth_of(body) > 0) {
        if (pos >= lines.size()) throw YamlError("yaml: unterminated '{' opened at line " + std::to_string(number));
        body += " " + lines[pos].text;
        pos++;
      }
      size_t at = 0;
      parse_flow_map(body, at, number, child);
      if (!trim(body.substr(at)).empty()) throw YamlError("yaml: trailing characters after '}' (line " + std::to_string(number) + ")");
    } else {
      child.kind = YamlNode::Scalar;
      child.scalar = unquote(val);
    }
    node.map[key] = child;
  }
}

bool parse_double(const std::string& s, double& out) {
  if (s.empty()) return false;
  char* end = nullptr;
  out = std::strtod(s.c_str(), &end);
  return end && *end == 0;
}
}  // namespace

const YamlNode& YamlNode::operator[](const std::string& key) const {
  if (kind != Map) return kNullNode;
  auto it = map.find(key);
  return it == map.end() ? kNullNode : it->second;
}

bool YamlNode::get(const std::string& key, bool dflt) const {
  const YamlNode& n = (*this)[key];
  if (n.kind != Scalar) return dflt;
  std::string s = n.scalar;
  std::transform(s.begin(), s.end(), s.begin(), ::tolower);
  if (s == "true" || s == "yes" || s == "on" || s == "y") return true;
  if (s == "false" || s == "no" || s == "off" || s == "n") return false;
  return dflt;
}
int YamlNode::get(const std::string& key, int dflt) const {
  const YamlNode& n = (*this)[key];
  double d;
  if (n.kind != Scalar || !parse_double(n.scalar, d)) return dflt;
  // a value no int holds (1e300, inf, nan): yaml-cpp's as<int>() throws BadConversion, which utils::get (utils.hpp:62-73) lets
  // through; the conversion itself would be undefined behaviour here (found by the sanitizer run of tests/test_host_fuzz.py)
  if (!(d >= -2147483648.0 && d <= 2147483647.0)) throw YamlError("yaml: '" + n.scalar + "' for '" + key + "' is not an integer in range");
  return (int)d;
}
double YamlNode::get(const std::string& key, double dflt) const {
  const YamlNode& n = (*this)[key];
  double d;
  if (n.kind != Scalar || !parse_double(n.scalar, d)) return dflt;
  return d;
}
std::string YamlNode::get(const std::string& key, const std::string& dflt) const {
  const YamlNode& n = (*this)[key];
  return n.kind == Scalar ? n.scalar : dflt;
}
std::vector<double> YamlNode::get_vector(const std::string& key) const {
  const YamlNode& n = (*this)[key];
  std::vector<double> out;
  if (n.kind != Sequence) return out;
  for (const std::string& s : n.seq) {
    double d;
    if (!parse_double(s, d)) throw YamlError("yaml: '" + s + "' in sequence '" + key + "' is not a number");
    out.push_back(d);
  }
  return out;
}

YamlNode yaml_parse(const std::string& text) {
  std::vector<Line> lines;
  std::istringstream ss(text);
  std::string raw;
  int number = 0;
  while (std::getline(ss, raw)) {
    number++;
    std::string s = strip_comment(raw);
    if (trim(s).empty()) continue;
    if (trim(s) == "---" || trim(s) == "...") continue;
    if (s.find('\t') != std::string::npos && s.find_first_not_of(" \t") > s.find('\t'))
      throw YamlError("yaml: tab used for indentation at line " + std::to_string(number));
    int indent = (int)s.find_first_not_of(' ');
    lines.push_back({indent, trim(s), number});
  }
  YamlNode root;
  root.kind = YamlNode::Map;
  size_t pos = 0;
  if (!lines.empty()) parse_block(lines, pos, lines[0].indent, root);
  if (pos != lines.size()) throw YamlError("yaml: unexpected dedent at line " + std::to_string(lines[pos].number));
  return root;
}

bool file_exists(const std::string& path) {
  std::ifstream f(path);
  return f.good();
}

YamlNode yaml_load_file(const std::string& path) {
  std::ifstream f(path);
  if (!f.good()) throw YamlError("yaml: cannot open " + path);
  std::stringstream ss;
  ss << f.rdbuf();
  return yaml_parse(ss.str());
}

}  // namespace rip
