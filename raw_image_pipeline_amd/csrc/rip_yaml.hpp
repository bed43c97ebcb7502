// rip_yaml.hpp -- the YAML-subset reader of the three configuration files.
#pragma once
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace rip {

// ---------------------------------------------------------------------------------------------
// Minimal YAML reader: nested block maps, scalars, flow sequences of scalars ("[a, b, c]",
// possibly spanning lines), comments.  Enough for the reference's three file kinds
// (config/pipeline_params_example.yaml, alphasense_calib_example.yaml,
// alphasense_color_calib_example.yaml).  Throws YamlError on malformed input.
// ---------------------------------------------------------------------------------------------
struct YamlError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct YamlNode {
  enum Kind { Null, Scalar, Sequence, Map } kind = Null;
  std::string scalar;
  std::vector<std::string> seq;
  std::map<std::string, YamlNode> map;

  const YamlNode& operator[](const std::string& key) const;  // Null node when absent
  bool defined() const { return kind != Null; }
  // utils::get<T>(node, key, default) (reference utils.hpp:61-74): value or default
  bool get(const std::string& key, bool dflt) const;
  int get(const std::string& key, int dflt) const;
  double get(const std::string& key, double dflt) const;
  std::string get(const std::string& key, const std::string& dflt) const;
  std::vector<double> get_vector(const std::string& key) const;  // empty when absent / not a sequence
};
YamlNode yaml_parse(const std::string& text);
YamlNode yaml_load_file(const std::string& path);  // throws YamlError when unreadable
bool file_exists(const std::string& path);

}  // namespace rip
