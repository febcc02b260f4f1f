// Test driver of tests/test_query_kind_cpu.py: the plan of a `movi query` command line (movi_amd/host/query_kind.hpp), printed without a GPU.
// stdin: one command line per line, without the program's name ("query -i idx -r reads.fq --zml --stdout").
// stdout, one line per case: every field of query_plan(parse_args(line)) --
//   kind=K prepare=P verdict_only= walk_only= result_vector= reserve_results= open_files= logs= logs_ignored= to_bpf=
//   report=SUFFIX mc_file= bpf=SUFFIX sa=SUFFIX matches=SUFFIX logs_stem=SUFFIX          ("-": no such file)
// or "rejected: MESSAGE" where parse_args refuses the line.  prepare: the MOVI_PREPARE_* value, "none" where nothing is prepared.
#include <iostream>
#include <sstream>

#include "../../movi_amd/host/options.cpp"
#include "../../movi_amd/host/query_kind.hpp"

using namespace movi_host;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::vector<std::string> words{"movi"};
        std::istringstream in(line);
        for (std::string w; in >> w;) words.push_back(w);
        std::vector<char *> argv;
        for (std::string &w : words) argv.push_back(&w[0]);
        try {
            const QueryPlan p = query_plan(parse_args((int)argv.size(), argv.data()));
            auto file = [](const std::string &s) { return s.empty() ? std::string("-") : s; };
            std::cout << "kind=" << query_kind_name(p.kind) << " prepare=" << (p.prepare == QueryPlan::kNoPrepare ? "none" : std::to_string(p.prepare))
                      << " verdict_only=" << p.verdict_only << " walk_only=" << p.walk_only << " result_vector=" << p.result_vector
                      << " reserve_results=" << p.reserve_results << " open_files=" << p.open_files << " logs=" << p.logs
                      << " logs_ignored=" << p.logs_ignored << " to_bpf=" << p.to_bpf << " report=" << file(p.report_suffix)
                      << " mc_file=" << p.mc_to_out_file << " bpf=" << file(p.bpf_suffix) << " sa=" << file(p.sa_suffix)
                      << " matches=" << file(p.matches_suffix) << " logs_stem=" << file(p.logs_stem) << "\n";
        } catch (const UsageError &e) {
            std::cout << "rejected: " << e.what() << "\n";
        }
    }
    return 0;
}
