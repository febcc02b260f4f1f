// query_kind.hpp -- which query a `movi query` command line runs, decided once: the engine entry point of a shard, the
// tables prepared with the index, the buffers a chunk needs and the files the command writes all follow from this plan.
// Plain C++ over options.hpp and the constants of include/movi_hip.h; tests/host/query_kind_driver.cpp prints it per command line.
#pragma once
#include <string>

#include "../../include/movi_hip.h"
#include "options.hpp"

namespace movi_host {

// One arm per query entry point of the engine, in the order the command tests for them: the first that applies is the query.
enum class QueryKind {
    PmlVerdictBins,   // --classify with --filter / --no-output: the bins are reduced on the GPU
    PmlLogs,          // --logs on a PML query that writes files
    MultiClassify,    // --multi-classify
    SaEntries,        // --sa-entries: the PML walk with a suffix-array entry per base
    Pml,
    Zml,
    Mem,
    Kmer,
    Count,
    KmerOcc,          // --kmer-occ: occurrences per k-mer (last: the arms above keep their numbers)
};

inline const char *query_kind_name(QueryKind k) {
    static const char *const names[] = {"pml_verdict_bins", "pml_logs", "multi_classify", "sa_entries", "pml", "zml", "mem", "kmer", "count", "kmer_occ"};
    return names[(int)k];
}

struct QueryPlan {
    QueryKind kind;
    int prepare;               // movi_index_prepare's `what`; kNoPrepare: nothing is prepared and no warm-up call is made
    static constexpr int kNoPrepare = -1;
    bool verdict_only;         // the verdicts' bins come back, never the PML vectors
    bool walk_only;            // the walk runs, no vector comes back
    bool result_vector;        // a chunk's PML / ZML vector is sized
    bool reserve_results;      // "reserve_host_results" is made beside the other reservations
    bool open_files;           // the query's own output files are opened under the prefix
    bool logs;                 // --logs is collected and written ...
    bool logs_ignored;         // ... or given where it is not collected: said once on stderr
    bool to_bpf;               // the vectors go to the BPF file
    // The files the command opens.  The prefix is -o's value, else <reads>.<index type>; the report always goes beside the reads.
    std::string report_suffix; // "<reads>.<index type>" + this: the classification report ("" = none, or it goes to stdout)
    bool mc_to_out_file;       // --multi-classify: the report is the -o file itself
    std::string bpf_suffix;    // prefix + this: the BPF file of a PML / ZML query
    std::string sa_suffix;     // prefix + this: the suffix-array entries beside it
    std::string matches_suffix;// prefix + this: the text file of a count, MEM, k-mer or k-mer occurrence query
    std::string logs_stem;     // prefix + this + ".costs" / ".scans" / ".fastforwards"
    bool locate;               // --locate on a count or MEM query: the shard also locates its hits (movi_locate_matches_host)
    std::string locs_suffix;   // prefix + this: their text positions, one line per line of the matches file ("" = none, or they go to stdout)
};

inline QueryPlan query_plan(const Options &o) {
    QueryPlan p;
    const bool out = o.write_output_allowed();
    // --logs runs on the first kernel, which uses none of the derived tables
    // (--mem: the count tables; --sa-entries: its own walk, no table of the PML walk)
    p.prepare = (o.pml && o.logs) ? QueryPlan::kNoPrepare
              : (int)(o.multi_classify ? MOVI_PREPARE_COLOR : o.sa_entries ? MOVI_PREPARE_SA : o.pml ? MOVI_PREPARE_PML : (o.zml ? MOVI_PREPARE_ZML : MOVI_PREPARE_COUNT));
    // --classify with --filter / --no-output needs verdicts only: the bins are reduced on the
    // GPU and the PML vectors never cross PCIe
    p.verdict_only = o.pml && o.classify && !out;                                      // PML only: ZML takes the host bins
    // `--no-output` without classification: the walk runs, nothing comes back (the engine is given a NULL vector)
    p.walk_only = o.ml() && !o.classify && (!out || o.multi_classify);                 // (--multi-classify: no vector comes back)
    p.result_vector = o.ml() && !p.verdict_only && !p.walk_only;
    p.reserve_results = o.ml() && (out || o.classify) && !(o.pml && o.classify && !out);
    p.open_files = (!o.write_stdout || o.classify) && out && !o.multi_classify;
    p.logs = o.logs && o.pml && p.open_files;
    p.logs_ignored = o.logs && !p.logs;
    p.to_bpf = o.ml() && out && !o.write_stdout_enabled();
    p.kind = p.verdict_only ? QueryKind::PmlVerdictBins
           : (o.pml && p.logs) ? QueryKind::PmlLogs
           : o.multi_classify ? QueryKind::MultiClassify
           : o.sa_entries ? QueryKind::SaEntries
           : o.pml ? QueryKind::Pml
           : o.zml ? QueryKind::Zml
           : o.mem ? QueryKind::Mem
           : o.kmer ? QueryKind::Kmer
           : o.kmer_occ ? QueryKind::KmerOcc : QueryKind::Count;
    if (o.classify && !o.filter && !o.write_stdout) p.report_suffix = "." + o.query_type() + ".report";   // src/classifier.cpp:39-61
    p.mc_to_out_file = o.multi_classify && !o.write_stdout && out;
    if (p.open_files) {
        if (o.kmer || o.kmer_occ) p.matches_suffix = "." + o.query_type() + "." + std::to_string(o.k);   // <out_file or reads.<index type>>.kmers.<k> (src/utils.cpp:348-366); --kmer-occ: .kmer_occ.<k>
        else if (o.mem) p.matches_suffix = ".mems";                                        // <out_file or reads.<index type>>.mems
        else if (o.ml()) {
            p.bpf_suffix = "." + o.query_type() + ".bpf";
            if (o.sa_entries) p.sa_suffix = "." + o.query_type() + ".sa_entries.bpf";      // src/utils.cpp:371-375: opened with the PML file, no BPF header
        } else p.matches_suffix = "." + o.query_type() + ".matches";
    }
    if (p.logs) p.logs_stem = "." + o.query_type();
    p.locate = o.locate && (o.count || o.mem);
    if (p.locate) {
        p.prepare |= (int)MOVI_PREPARE_SA;                                                 // (kind Count / Mem: MOVI_PREPARE_COUNT so far)
        if (p.open_files) p.locs_suffix = p.matches_suffix + ".locs";
    }
    return p;
}

}  // namespace movi_host
