// A small JSON document model for sfm_data.json (host code only; shared by adjust.hip and adjust_cli.cpp).
// parse() keeps object keys in file order and tells integers from floats; dump() writes a value exactly as Python's
// json.dump does with its defaults: ", " and ": " separators, ensure_ascii (lower-case \uXXXX escapes), floats as
// repr() (Infinity / -Infinity / NaN for the non-finite ones), integers as written.  A repeated key keeps its first
// position and its last value, as a Python dict does.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace sfmjson {

struct Value {
  enum Kind { Null, False, True, Int, Float, Str, Arr, Obj } kind = Null;
  std::string s;  // Str: UTF-8 text; Int: the digits (Python ints are unbounded)
  double d = 0.0;
  std::vector<Value> a;
  std::vector<std::pair<std::string, Value>> o;

  const Value *get(const char *k) const {
    for (const auto &kv : o)
      if (kv.first == k) return &kv.second;
    return nullptr;
  }
  Value *get(const char *k) {
    for (auto &kv : o)
      if (kv.first == k) return &kv.second;
    return nullptr;
  }
  bool is_num() const { return kind == Int || kind == Float; }
  double num() const { return kind == Int ? strtod(s.c_str(), nullptr) : d; }
  static Value make_float(double v) {
    Value x;
    x.kind = Float;
    x.d = v;
    return x;
  }
  static Value make_arr() {
    Value x;
    x.kind = Arr;
    return x;
  }
};

// a double as Python's repr() writes it: the shortest text that reads back as the same double; positional notation for
// decimal exponents -4 < e <= 16 (with ".0" for an integer), else d[.ddd]e+XX
inline std::string py_repr(double v) {
  if (std::isnan(v)) return "nan";
  if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
  if (v == 0.0) return std::signbit(v) ? "-0.0" : "0.0";
  char buf[64];
  for (int p = 1; p <= 17; ++p) {
    snprintf(buf, sizeof buf, "%.*e", p - 1, v);
    if (strtod(buf, nullptr) == v) break;
  }
  std::string s(buf);
  const bool neg = s[0] == '-';
  if (neg) s = s.substr(1);
  const size_t e = s.find('e');
  const int exp10 = atoi(s.c_str() + e + 1);
  std::string digits;
  for (size_t i = 0; i < e; ++i)
    if (s[i] != '.') digits += s[i];
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  const int decpt = exp10 + 1;
  std::string out;
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0) out = "0." + std::string(-decpt, '0') + digits;
    else if (decpt >= (int)digits.size()) out = digits + std::string(decpt - digits.size(), '0') + ".0";
    else out = digits.substr(0, decpt) + "." + digits.substr(decpt);
  } else {
    out = digits.substr(0, 1);
    if (digits.size() > 1) out += "." + digits.substr(1);
    char eb[16];
    snprintf(eb, sizeof eb, "e%c%02d", exp10 < 0 ? '-' : '+', exp10 < 0 ? -exp10 : exp10);
    out += eb;
  }
  return (neg ? "-" : "") + out;
}

namespace detail {

struct Parser {
  const char *p, *end;
  std::string err;
  void ws() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool fail(const char *what) {
    if (err.empty()) err = what;
    return false;
  }
  bool lit(const char *w) {
    const size_t n = strlen(w);
    if ((size_t)(end - p) < n || memcmp(p, w, n) != 0) return false;
    p += n;
    return true;
  }
  static void put_utf8(std::string *s, uint32_t c) {  // (lone surrogates go through as 3-byte sequences)
    if (c < 0x80) {
      *s += (char)c;
    } else if (c < 0x800) {
      *s += (char)(0xC0 | (c >> 6));
      *s += (char)(0x80 | (c & 0x3F));
    } else if (c < 0x10000) {
      *s += (char)(0xE0 | (c >> 12));
      *s += (char)(0x80 | ((c >> 6) & 0x3F));
      *s += (char)(0x80 | (c & 0x3F));
    } else {
      *s += (char)(0xF0 | (c >> 18));
      *s += (char)(0x80 | ((c >> 12) & 0x3F));
      *s += (char)(0x80 | ((c >> 6) & 0x3F));
      *s += (char)(0x80 | (c & 0x3F));
    }
  }
  bool hex4(uint32_t *c) {
    if (end - p < 4) return fail("truncated \\u escape");
    *c = 0;
    for (int i = 0; i < 4; ++i) {
      const char h = *p++;
      *c <<= 4;
      if (h >= '0' && h <= '9') *c |= (uint32_t)(h - '0');
      else if (h >= 'a' && h <= 'f') *c |= (uint32_t)(h - 'a' + 10);
      else if (h >= 'A' && h <= 'F') *c |= (uint32_t)(h - 'A' + 10);
      else return fail("bad \\u escape");
    }
    return true;
  }
  bool str(std::string *out) {
    if (p >= end || *p != '"') return fail("expected a string");
    ++p;
    out->clear();
    while (p < end && *p != '"') {
      const unsigned char ch = (unsigned char)*p;
      if (ch < 0x20) return fail("control character in a string");
      if (ch != '\\') {
        *out += (char)ch;
        ++p;
        continue;
      }
      if (++p >= end) return fail("truncated escape");
      const char e = *p++;
      switch (e) {
        case '"': *out += '"'; break;
        case '\\': *out += '\\'; break;
        case '/': *out += '/'; break;
        case 'b': *out += '\b'; break;
        case 'f': *out += '\f'; break;
        case 'n': *out += '\n'; break;
        case 'r': *out += '\r'; break;
        case 't': *out += '\t'; break;
        case 'u': {
          uint32_t c;
          if (!hex4(&c)) return false;
          if (c >= 0xD800 && c < 0xDC00 && end - p >= 6 && p[0] == '\\' && p[1] == 'u') {
            const char *save = p;
            p += 2;
            uint32_t lo;
            if (!hex4(&lo)) return false;
            if (lo >= 0xDC00 && lo < 0xE000) c = 0x10000 + ((c - 0xD800) << 10) + (lo - 0xDC00);
            else p = save;
          }
          put_utf8(out, c);
          break;
        }
        default: return fail("bad escape");
      }
    }
    if (p >= end) return fail("unterminated string");
    ++p;
    return true;
  }
  bool number(Value *v) {
    const char *b = p;
    if (p < end && *p == '-') ++p;
    if (lit("Infinity")) {
      v->kind = Value::Float;
      v->d = *b == '-' ? -INFINITY : INFINITY;
      return true;
    }
    if (p >= end || !(*p >= '0' && *p <= '9')) return fail("bad number");
    if (*p == '0') ++p;
    else
      while (p < end && *p >= '0' && *p <= '9') ++p;
    bool is_float = false;
    if (p < end && *p == '.') {
      is_float = true;
      ++p;
      if (p >= end || !(*p >= '0' && *p <= '9')) return fail("bad number");
      while (p < end && *p >= '0' && *p <= '9') ++p;
    }
    if (p < end && (*p == 'e' || *p == 'E')) {
      is_float = true;
      ++p;
      if (p < end && (*p == '+' || *p == '-')) ++p;
      if (p >= end || !(*p >= '0' && *p <= '9')) return fail("bad number");
      while (p < end && *p >= '0' && *p <= '9') ++p;
    }
    const std::string t(b, p);
    if (is_float) {
      v->kind = Value::Float;
      v->d = strtod(t.c_str(), nullptr);
    } else {
      v->kind = Value::Int;
      v->s = (t == "-0") ? std::string("0") : t;
    }
    return true;
  }
  bool value(Value *v, int depth) {
    if (depth > 512) return fail("nesting too deep");
    ws();
    if (p >= end) return fail("unexpected end");
    const char c = *p;
    if (c == '{') {
      ++p;
      v->kind = Value::Obj;
      ws();
      if (p < end && *p == '}') {
        ++p;
        return true;
      }
      for (;;) {
        ws();
        std::string k;
        if (!str(&k)) return false;
        ws();
        if (p >= end || *p != ':') return fail("expected ':'");
        ++p;
        Value x;
        if (!value(&x, depth + 1)) return false;
        Value *dup = v->get(k.c_str());
        if (dup) *dup = std::move(x);
        else v->o.emplace_back(std::move(k), std::move(x));
        ws();
        if (p < end && *p == ',') {
          ++p;
          continue;
        }
        if (p < end && *p == '}') {
          ++p;
          return true;
        }
        return fail("expected ',' or '}'");
      }
    }
    if (c == '[') {
      ++p;
      v->kind = Value::Arr;
      ws();
      if (p < end && *p == ']') {
        ++p;
        return true;
      }
      for (;;) {
        v->a.emplace_back();
        if (!value(&v->a.back(), depth + 1)) return false;
        ws();
        if (p < end && *p == ',') {
          ++p;
          continue;
        }
        if (p < end && *p == ']') {
          ++p;
          return true;
        }
        return fail("expected ',' or ']'");
      }
    }
    if (c == '"') {
      v->kind = Value::Str;
      return str(&v->s);
    }
    if (lit("true")) {
      v->kind = Value::True;
      return true;
    }
    if (lit("false")) {
      v->kind = Value::False;
      return true;
    }
    if (lit("null")) {
      v->kind = Value::Null;
      return true;
    }
    if (lit("NaN")) {
      v->kind = Value::Float;
      v->d = NAN;
      return true;
    }
    return number(v);
  }
};

inline void dump_str(const std::string &s, std::string *out) {
  *out += '"';
  size_t i = 0;
  char buf[16];
  while (i < s.size()) {
    const unsigned char c = (unsigned char)s[i];
    uint32_t cp = c;
    size_t n = 1;
    if (c >= 0xF0 && i + 3 < s.size() + 0) {
      cp = ((c & 0x07u) << 18) | (((unsigned char)s[i + 1] & 0x3Fu) << 12) | (((unsigned char)s[i + 2] & 0x3Fu) << 6) |
           ((unsigned char)s[i + 3] & 0x3Fu);
      n = 4;
    } else if (c >= 0xE0 && i + 2 < s.size()) {
      cp = ((c & 0x0Fu) << 12) | (((unsigned char)s[i + 1] & 0x3Fu) << 6) | ((unsigned char)s[i + 2] & 0x3Fu);
      n = 3;
    } else if (c >= 0xC0 && i + 1 < s.size()) {
      cp = ((c & 0x1Fu) << 6) | ((unsigned char)s[i + 1] & 0x3Fu);
      n = 2;
    }
    i += n;
    if (cp == '"') *out += "\\\"";
    else if (cp == '\\') *out += "\\\\";
    else if (cp == '\n') *out += "\\n";
    else if (cp == '\r') *out += "\\r";
    else if (cp == '\t') *out += "\\t";
    else if (cp == '\b') *out += "\\b";
    else if (cp == '\f') *out += "\\f";
    else if (cp >= 0x20 && cp < 0x7F) *out += (char)cp;
    else if (cp < 0x10000) {
      snprintf(buf, sizeof buf, "\\u%04x", cp);
      *out += buf;
    } else {
      const uint32_t v = cp - 0x10000;
      snprintf(buf, sizeof buf, "\\u%04x\\u%04x", 0xD800 + (v >> 10), 0xDC00 + (v & 0x3FF));
      *out += buf;
    }
  }
  *out += '"';
}

}  // namespace detail

inline bool parse(const std::string &text, Value *out, std::string *err) {
  detail::Parser P{text.data(), text.data() + text.size(), std::string()};
  *out = Value();
  bool ok = P.value(out, 0);
  if (ok) {
    P.ws();
    if (P.p != P.end) ok = P.fail("extra data after the document");
  }
  if (!ok && err) *err = P.err + " at byte " + std::to_string((long long)(P.p - text.data()));
  return ok;
}

inline void dump(const Value &v, std::string *out) {
  switch (v.kind) {
    case Value::Null: *out += "null"; return;
    case Value::False: *out += "false"; return;
    case Value::True: *out += "true"; return;
    case Value::Int: *out += v.s; return;
    case Value::Float:
      if (std::isnan(v.d)) *out += "NaN";
      else if (std::isinf(v.d)) *out += v.d < 0 ? "-Infinity" : "Infinity";
      else *out += py_repr(v.d);
      return;
    case Value::Str: detail::dump_str(v.s, out); return;
    case Value::Arr:
      *out += '[';
      for (size_t i = 0; i < v.a.size(); ++i) {
        if (i) *out += ", ";
        dump(v.a[i], out);
      }
      *out += ']';
      return;
    case Value::Obj:
      *out += '{';
      for (size_t i = 0; i < v.o.size(); ++i) {
        if (i) *out += ", ";
        detail::dump_str(v.o[i].first, out);
        *out += ": ";
        dump(v.o[i].second, out);
      }
      *out += '}';
      return;
  }
}

inline bool read_file(const char *path, std::string *out) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  out->clear();
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
  const bool ok = !ferror(f);
  fclose(f);
  return ok;
}

inline bool write_file(const char *path, const std::string &text) {
  FILE *f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  return fclose(f) == 0 && ok;
}

}  // namespace sfmjson
