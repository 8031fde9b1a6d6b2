// The read -> primer table of --meta --amplicon-depth (extractReadSequences, src/mgsr.cpp:1216-1342), host only.  Despite the
// option's name the file maps read identifiers to primer identifiers: one `read id <TAB> primer id` per line.  Groups are
// numbered by the first appearance of the primer id; a read id listed twice belongs to the primer of its last line (the
// earlier primer keeps its group, possibly empty); empty lines are skipped.
// Not reproduced: for a line without exactly two tab-separated non-empty fields the reference prints an error and goes on with
// the values left over from the previous line.  Here such a line is PMX_ERR_FORMAT with its line number.
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../api_internal.hpp"

struct pmx_amplicons {
    std::vector<std::string> groups;                    // primer ids by first appearance
    std::unordered_map<std::string, int32_t> group_of;  // primer id -> group
    std::unordered_map<std::string, int32_t> of_read;   // read id -> group
};

extern "C" {

int pmx_amplicons_load(const char* path, pmx_amplicons** out) {
    if (!path || !out) return PMX_ERR_ARG;
    std::ifstream in(path);
    std::string line;
    bool any = in.is_open() && std::getline(in, line);
    if (!in.is_open() || (!any && !in.eof())) {   // (a directory opens and fails on the first read)
        pmx::set_error(std::string("cannot read ") + path);
        return PMX_ERR_IO;
    }
    pmx_amplicons* a = new pmx_amplicons();
    for (int64_t number = 1; any; any = (bool)std::getline(in, line), ++number) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 == line.size() || line.find('\t', tab + 1) != std::string::npos) {
            pmx::set_error(std::string(path) + ": line " + std::to_string(number) + " does not have exactly two tab-separated non-empty fields (read id, primer id)");
            delete a;
            return PMX_ERR_FORMAT;
        }
        const std::string primer = line.substr(tab + 1);
        const auto at = a->group_of.emplace(primer, (int32_t)a->groups.size());
        if (at.second) a->groups.push_back(primer);
        a->of_read[line.substr(0, tab)] = at.first->second;
    }
    *out = a;
    return PMX_OK;
}

void pmx_amplicons_free(pmx_amplicons* a) { delete a; }

int32_t pmx_amplicons_num_groups(const pmx_amplicons* a) { return a ? (int32_t)a->groups.size() : 0; }

const char* pmx_amplicons_group_name(const pmx_amplicons* a, int32_t g) {
    return a && g >= 0 && (size_t)g < a->groups.size() ? a->groups[(size_t)g].c_str() : nullptr;
}

int32_t pmx_amplicons_lookup(const pmx_amplicons* a, const char* read_name) {
    if (!a || !read_name) return -1;
    const auto at = a->of_read.find(read_name);
    return at == a->of_read.end() ? -1 : at->second;
}

}  // extern "C"
