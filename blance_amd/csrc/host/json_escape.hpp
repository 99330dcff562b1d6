// encoding/json's string escaping (encodeState.string with escapeHTML = true) and Go's UTF-8 validity rule, shared by the
// PartitionMap codec (blance_wire.cpp) and the planner library (blance_plan_wire_names escapes every name once, then the
// device composes documents from the escaped forms): one copy, so both produce the same bytes.  Host only, header only.
#pragma once

#include <stddef.h>

#include <string>

namespace blance_json {

// length of the valid UTF-8 sequence at q (0 if invalid), Go's utf8.DecodeRune rules
inline int utf8_len(const unsigned char* q, const unsigned char* end) {
    unsigned char c = q[0];
    if (c < 0x80) return 1;
    if (c < 0xC2) return 0;
    if (c < 0xE0) return (end - q >= 2 && (q[1] & 0xC0) == 0x80) ? 2 : 0;
    if (c < 0xF0) {
        if (end - q < 3 || (q[1] & 0xC0) != 0x80 || (q[2] & 0xC0) != 0x80) return 0;
        if (c == 0xE0 && q[1] < 0xA0) return 0;
        if (c == 0xED && q[1] > 0x9F) return 0;          // surrogates
        return 3;
    }
    if (c < 0xF5) {
        if (end - q < 4 || (q[1] & 0xC0) != 0x80 || (q[2] & 0xC0) != 0x80 || (q[3] & 0xC0) != 0x80) return 0;
        if (c == 0xF0 && q[1] < 0x90) return 0;
        if (c == 0xF4 && q[1] > 0x8F) return 0;
        return 4;
    }
    return 0;
}

// appends the JSON string of s[0 .. n), quotes included
inline void put_string(std::string& o, const char* s, size_t n) {     // encodeState.string, escapeHTML = true
    static const char kHex[] = "0123456789abcdef";
    o.push_back('"');
    size_t start = 0, i = 0;
    const unsigned char* u = (const unsigned char*)s;
    while (i < n) {
        unsigned char c = u[i];
        if (c < 0x80) {
            if (c >= 0x20 && c != '"' && c != '\\' && c != '<' && c != '>' && c != '&') { i++; continue; }
            o.append(s + start, i - start);
            switch (c) {
                case '"': o += "\\\""; break;
                case '\\': o += "\\\\"; break;
                case '\b': o += "\\b"; break;
                case '\f': o += "\\f"; break;
                case '\n': o += "\\n"; break;
                case '\r': o += "\\r"; break;
                case '\t': o += "\\t"; break;
                default:
                    o += "\\u00";
                    o.push_back(kHex[c >> 4]);
                    o.push_back(kHex[c & 0xF]);
            }
            i++;
            start = i;
            continue;
        }
        int l = utf8_len(u + i, u + n);
        if (l == 0) {
            o.append(s + start, i - start);
            o += "\\ufffd";
            i++;
            start = i;
            continue;
        }
        if (l == 3 && u[i] == 0xE2 && u[i + 1] == 0x80 && (u[i + 2] == 0xA8 || u[i + 2] == 0xA9)) {   // U+2028 / U+2029
            o.append(s + start, i - start);
            o += "\\u202";
            o.push_back(kHex[u[i + 2] & 0xF]);
            i += 3;
            start = i;
            continue;
        }
        i += (size_t)l;
    }
    o.append(s + start, n - start);
    o.push_back('"');
}

}  // namespace blance_json
