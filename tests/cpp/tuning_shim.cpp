// A few lines around popsift_amd/csrc/hip/psx_tuning.h for tests/test_tuning_cpu.py: built with the host compiler, loaded
// with ctypes.  Every call walks the table once, as psx_create does.
#include "psx_tuning.h"

#include <cstdio>
#include <cstring>

namespace {
long long as_ll(long long v) { return v; }
long long as_ll(const std::string&) { return 0; }
std::string as_text(long long v) { return std::to_string(v); }
std::string as_text(const std::string& v) { return v; }
void put(char* out, int cap, const std::string& s) { if (out && cap > 0) snprintf(out, (size_t)cap, "%s", s.c_str()); }
} // namespace

extern "C" {

// the field of the row `env_name` after psx_tuning_from_env: *value (0 for a STR row), text (the value as text), error (the
// parser's error text, empty when there is none).  Returns 0, or 1 when the table has no such row.
int tuning_get(const char* env_name, long long* value, char* text, int text_cap, char* error, int error_cap)
{
    std::string err;
    const PsxTuning t = psx_tuning_from_env(&err);
    put(error, error_cap, err);
#define X(kind, type, field, env, dflt, accept, doc) \
    if (strcmp(env_name, env) == 0) { *value = as_ll(t.field); put(text, text_cap, as_text(t.field)); return 0; }
    PSX_TUNING_TABLE(X)
#undef X
    return 1;
}

// one line per row of the table: "<environment name> <kind> <default>"
int tuning_rows(char* out, int cap)
{
    std::string s;
    const PsxTuning d;
#define X(kind, type, field, env, dflt, accept, doc) s += std::string(env) + " " + #kind + " " + as_text(d.field) + "\n";
    PSX_TUNING_TABLE(X)
#undef X
    put(out, cap, s);
    return (int)s.size();
}

}
