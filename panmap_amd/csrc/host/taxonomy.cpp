// The taxonomic metadata table of --meta --filter-and-assign (loadTaxonomicMetadata, src/mgsr.cpp:198-256), host only.
#include <fstream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../api_internal.hpp"

struct pmx_taxonomy {
    std::vector<std::string> taxa;                      // by first appearance
    std::unordered_map<std::string, int64_t> taxon_of;  // taxon name -> index
    std::unordered_map<std::string, int64_t> of_id;     // node identifier -> taxon index
};

extern "C" {

int pmx_taxonomy_load(const char* path, const char* rank, pmx_taxonomy** out) {
    if (!path || !rank || !out) return PMX_ERR_ARG;
    std::ifstream in(path);
    std::string line;
    const bool header_read = in.is_open() && std::getline(in, line);
    if (!in.is_open() || (!header_read && !in.eof())) {   // (a directory opens and fails on the first read)
        pmx::set_error(std::string("cannot read ") + path);
        return PMX_ERR_IO;
    }
    if (!header_read) { pmx::set_error(std::string(path) + ": no header line"); return PMX_ERR_FORMAT; }
    int column = -1;
    {
        std::istringstream header(line);
        std::string name;
        for (int i = 0; header >> name; ++i)
            if (name == rank) { column = i; break; }
    }
    if (column <= 0) {   // (the first column holds the identifiers)
        pmx::set_error(std::string("taxonomic rank '") + rank + "' not found in the header of " + path + (column == 0 ? " past its first column" : ""));
        return PMX_ERR_ARG;
    }
    pmx_taxonomy* t = new pmx_taxonomy();
    while (std::getline(in, line)) {
        std::istringstream row(line);
        std::string id, taxon;
        if (!(row >> id)) continue;
        for (int i = 1; i <= column; ++i)
            if (!(row >> taxon)) {
                pmx::set_error(std::string(path) + ": the row of '" + id + "' has fewer than " + std::to_string(column + 1) + " columns");
                delete t;
                return PMX_ERR_FORMAT;
            }
        if (taxon == ".") continue;
        const auto at = t->taxon_of.emplace(taxon, (int64_t)t->taxa.size());
        if (at.second) t->taxa.push_back(taxon);
        t->of_id[id] = at.first->second;
    }
    *out = t;
    return PMX_OK;
}

void pmx_taxonomy_free(pmx_taxonomy* t) { delete t; }

int64_t pmx_taxonomy_num_taxa(const pmx_taxonomy* t) { return t ? (int64_t)t->taxa.size() : 0; }

const char* pmx_taxonomy_taxon_name(const pmx_taxonomy* t, int64_t taxon) {
    return t && taxon >= 0 && (size_t)taxon < t->taxa.size() ? t->taxa[(size_t)taxon].c_str() : nullptr;
}

int64_t pmx_taxonomy_lookup(const pmx_taxonomy* t, const char* identifier) {
    if (!t || !identifier) return -1;
    const auto at = t->of_id.find(identifier);
    return at == t->of_id.end() ? -1 : at->second;
}

}  // extern "C"
