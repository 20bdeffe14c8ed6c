// fqc_tool -- the reference's two commands over the GPU block farm (fqcomp28_amd/csrc/process.hpp):
//   fqc_tool c <in.fastq> <out.fqc> [-t threads] [-R block MiB] [-S sample MiB] [-d dev,dev,...] [--accumulate-n]
//              [--index [--index-stride Ki symbols, a multiple of 64]]   (extension: decode indexes in <out.fqc>.fqx)
//              [--checksum]   (extension: the CRC-32 of every chunk and of the whole file in <out.fqc>.fqs; the archive itself
//               is what it is without the option.  For input with bare '+' lines the file's value is zlib's CRC-32 of <in.fastq>)
//   fqc_tool d <in.fqc> <out.fastq> [-t threads] [-d dev,dev,...] [--records A:B] [--index [--index-stride Ki]]
//              (extension: --records restores records A .. B-1 only, numbered from 0 across the archive; A: = to the end)
//              (extension: --index also leaves <in.fqc>.fqx behind if no usable one lies there: restore and index in one pass;
//               --records never builds)
//              (extension: with <in.fqc>.fqs beside the archive every restored chunk is verified before it is written: a chunk
//               whose digest differs ends the command, exit 1, no output.  A .fqs that is damaged, unclosed or another archive's
//               is reported and not used; --records never verifies)
//   fqc_tool d <in.fqc> <out.fasta> --fasta [-t threads] [-d dev,dev,...] [--records A:B]
//              (extension: the sequences alone, as FASTA -- per record ">" + the header line without its '@', the bases on one
//               line, N as N.  The quality streams are not read from the archive, not uploaded and not decoded, so damage to
//               them goes unseen.  Uses <in.fqc>.fqx when it lies there (its sequence indexes); never builds one, never
//               verifies: --fasta with --index or --index-stride, or with c, x or t, is a usage error.  A failed run leaves
//               neither <out.fasta> nor <out.fasta>.part)
//   fqc_tool d <in.fqc> <out.fastq> [-t threads] [-d dev,dev,...] [--min-len N] [--max-len N] [--max-n K] [--min-mean-q Q] [--max-low-q Q:PCT]
//              (extension: any of these restores only the reads that pass, in input order, as the bytes a plain restore writes
//               for them: length N .. N, at most K bases N, floor(mean Phred) at least Q, at most PCT percent of the Phred
//               values below Q.  The reads are judged and gathered on the device where the decode left the chunk; only the kept
//               bytes come down.  <in.fqc>.fqx is used and <in.fqc>.fqs verified -- against the whole chunk, before any of it is
//               written -- when they lie there.  A filter with c, x, t or s, with --records, --fasta, --index or --index-stride,
//               a value out of range and a malformed Q:PCT are usage errors.  A failed run leaves neither <out.fastq> nor
//               <out.fastq>.part)
//   fqc_tool d <in.fqc> <out.fastq> [-t threads] [-d dev,dev,...] [--cut-front N] [--cut-tail N] [--trim-q5 Q] [--trim-q3 Q] [--crop L]
//              (extension: any of these restores the reads TRIMMED, with or without the filter options, which then judge what
//               is left: N bases cut from the 5' / the 3' end first, then the low-quality 5' / 3' end cut by the running-sum
//               rule of BWA -q / cutadapt -q with cutoff Q, then at most L bases kept from the new front.  A read of which
//               nothing is left is dropped.  Trimmed and gathered on the device as the filter is, .fqx used and .fqs verified
//               the same way.  A trim option with c, x, t or s, with --records, --fasta, --index or --index-stride, N above
//               65535, Q above 64 and --crop 0 are usage errors.  A failed run leaves neither <out.fastq> nor <out.fastq>.part)
//   fqc_tool d <in.fqc> <out.fastq> [-t threads] [-d dev,dev,...] --adapter SEQ [--adapter-overlap N] [--adapter-err PCT]
//              (extension: restores the reads with the 3' adapter SEQ (1 .. 64 of ACGT) CLIPPED, with or without the trim and
//               filter options, which then work on what is left in front of the adapter: the read is cut at the leftmost place
//               where SEQ, or the part of it that fits in front of the read's end, at least N bases of it (default 5, at most
//               SEQ's length), matches with at most PCT percent mismatches (default 10, at most 50; an N in the read is a
//               mismatch, no indels).  A read that starts with the adapter is dropped.  Searched, trimmed and gathered on the
//               device, .fqx used and .fqs verified as with a trim.  An adapter option with c, x, t or s, with --records,
//               --fasta, --index or --index-stride, without --adapter, and an adapter fqgpu_adapter_check refuses are usage
//               errors.  A failed run leaves neither <out.fastq> nor <out.fastq>.part)
//   fqc_tool d <in.fqc> <out.fastq> [-t threads] [-d dev,dev,...] [--poly-g [N] | --poly-x [N]] [--poly-every K] [--poly-mism M]
//              [--window W:Q]
//              (extension: restores the reads with their POLY-G TAIL (--poly-x: a tail of any one base) and everything from a
//               SLIDING-WINDOW quality drop on cut, with or without --adapter, the trim and the filter options; both stand
//               behind the adapter clip and in front of the trim.  The tail: the longest run at the 3' end, at least N bases
//               (default 10, 1 .. 65535), that begins and ends with the base and has at most one other base per K (default 8,
//               2 .. 255) and M in all (default 5, 0 .. 255); the walk from the end stops at the first place with more.  The
//               window (Trimmomatic SLIDINGWINDOW:W:Q, fastp --cut_right): behind --cut-front / --cut-tail, the read is cut in
//               the first window of W bases (1 .. 32) whose mean Phred is below Q (1 .. 64), at its first base below Q.
//               Found, trimmed and gathered on the device, .fqx used and .fqs verified as with a trim.  One of these options
//               with c, x, t or s, with --records, --fasta, --index or --index-stride, --poly-every or --poly-mism without
//               --poly-g or --poly-x, and values fqgpu_tail_check refuses are usage errors.  A failed run leaves neither
//               <out.fastq> nor <out.fastq>.part.  N is optional: the argument behind --poly-g / --poly-x is taken for it
//               whenever it does not begin with '-', so a word that is no number there is a usage error, not a path)
//   fqc_tool d <in1.fqc> <out1.fastq> --mate <in2.fqc> <out2.fastq> [--adapter2 SEQ] [-t threads] [-d dev,dev,...]
//              [every filter, trim, adapter, poly and window option]
//              (extension: PAIRED restore -- two archives whose records are mates, restored in step: record i of both outputs
//               are mates, and a pair is written only if BOTH mates pass, so the outputs stay in step whatever is dropped.
//               Every selection option applies to both mates; --adapter2 is mate 2's 3' adapter (default: --adapter's).  The
//               read ids of every pair -- the header line up to its first blank, without a "/1" or "/2" at the end -- are
//               compared on the device: the first pair whose ids differ ends the command, exit 1, naming the record.  Without
//               a selection option both files are restored whole and only the ids are checked.  The archives need the same
//               number of records and nothing else: different block sizes, read lengths and header formats are fine, a chunk
//               of <in2.fqc> that straddles a chunk boundary of <in1.fqc> is decoded twice.  Each archive's .fqx is used and
//               its .fqs verified as in a single restore.  --mate with c, x, t or s, with --records, --fasta, --index or
//               --index-stride, and --adapter2 without --mate or without --adapter's rules met are usage errors.
//               [--overlap-trim] [--overlap-report <file.tsv>] [--overlap-min N] [--overlap-mism M] [--overlap-err PCT]: the mate
//               overlap (include/fqgpu.h: where the two mates stop being reverse complements of each other is the fragment's
//               end, no adapter sequence needed).  --overlap-trim cuts both mates there, in front of every other step;
//               --overlap-report writes the summary and the insert-size histogram of the overlapping pairs as text, the same
//               bytes whatever -t, -R and .fqx; either turns the analysis on, the other three (defaults 30, 5, 20) set its spec.
//               With the report alone both output files are what they are without it.  Any of the five without --mate, the
//               last three without one of the first two, and a spec fqgpu_overlap_check refuses are usage errors.  A failed run
//               leaves neither output nor a .part file.
//               [--overlap-correct] [--correct-q GOOD:BAD]: OVERLAP CORRECTION (include/fqgpu.h, fastp's --correction) -- where
//               the mates disagree inside their overlap and one base has a Phred of GOOD or more while the other has BAD or
//               less (default 30:14), the poor base and its quality are replaced by the confident one's, on the device, behind
//               the overlap's search and in front of every step that judges either mate.  An overlap option in its own
//               right: it turns the analysis on, alone or beside any other option of d --mate, and the three spec options
//               may be given with it alone.  --overlap-correct without --mate, --correct-q without --overlap-correct and a
//               pair fqgpu_correct_check refuses (GOOD 1 .. 63, BAD below GOOD) are usage errors.
//               [--merge <merged.fastq>] [--merge-min-len N] [--merge-floor-q Q]: MATE MERGING (include/fqgpu.h, fastp's --merge,
//               FLASH) -- a pair whose mates overlap (it has an insert size I of N or more, default 1) and both pass the
//               selection exactly as they would without the option is written as ONE read of I bases to <merged.fastq> and to
//               neither mate file: mate 1's header line, the fragment from its first base to its last, in the overlap the
//               consensus of the two mates (where they differ the base with the higher Phred, its Phred the difference, Q at the
//               least, default 2).  Built on the device from the untrimmed, possibly corrected mates; the merged file's bytes do
//               not depend on -t, -R or .fqx.  An overlap option in its own right, as --overlap-correct is.  In "mate1" /
//               "mate2" a merged pair shows under "dropped_unmarked".  --merge without --mate, --merge-min-len or --merge-floor-q
//               without --merge, a spec fqgpu_merge_check refuses (N 1 .. 1023, Q 0 .. 63) and --merge with --cut-front,
//               --cut-tail or --crop -- positional cuts have no defined meaning on a merged read yet -- are usage errors.  A
//               failed run leaves none of the three outputs and no .part file)
//   fqc_tool x <in.fqc> [-t threads] [-d dev,dev,...] [--index-stride Ki]
//              (extension: builds <in.fqc>.fqx for an archive written without --index, by another writer of the format, or
//               whose index file is lost, stale or damaged: one serial decode of every block, nothing restored; always
//               builds afresh and replaces the old file once the last block has succeeded)
//   fqc_tool t <in.fqc> [-t threads] [-d dev,dev,...]
//              (extension: decodes every block, restores nothing, writes no file; compares every chunk with <in.fqc>.fqs --
//               exit 1 at the first that differs, and when the .fqs is there but cannot be used or the archive's size is not
//               the recorded one.  Without a .fqs the streams are still decoded: "sums": "none", a warning, exit 0.  Uses
//               <in.fqc>.fqx when it lies there)
//   fqc_tool s <in.fqc> <report.tsv> [-t threads] [-d dev,dev,...] [--positions P]
//              (extension: everything t does -- same checks, same exit codes, <in.fqc>.fqx and <in.fqc>.fqs used when they lie
//               there -- and a read summary of the archive, taken on the device where each chunk's decode left it: records,
//               bases, read lengths, reads with N, and per position in the read (rows 0 .. P - 1, row P = every position >= P;
//               default P 512) the counts of A C G T N and of every Phred value; histograms of the reads' mean quality and GC
//               percentage.  Text, tab-separated, integers only; written as <report.tsv>.part and renamed on success, a failed
//               run leaves neither)
//   fqc_tool c <in.fastq> <out.fqc> ... --stats <report.tsv> [--positions P]
//              (extension: the same report for the input, taken beside the encode; the archive is what it is without the
//               option, and `s` on it gives the same bytes.  --stats with d, x or t, and --positions without a report to
//               write, are usage errors)
//   fqc_tool s <in.fqc> <report.tsv> ... --adapters LIST [--adapter-overlap N] [--adapter-err PCT]
//   fqc_tool c <in.fastq> <out.fqc> ... --stats <report.tsv> --adapters LIST [--adapter-overlap N] [--adapter-err PCT]
//              (extension: ADAPTER CONTENT -- the report also says, for each of up to 16 probe adapters, in how many reads
//               `d --adapter` with that sequence would find it, how many bases it would cut, in how many reads the whole probe
//               shows, how many it would empty, and the reads by the place of the cut (--positions rows, as the summary); the
//               same for "any", the leftmost cut of all probes.  Searched on the device beside the summary, all probes in one
//               pass.  LIST is comma-separated; an item is `all` (every built-in), a built-in name -- truseq, truseq-r1,
//               truseq-r2, nextera, smallrna-3p, smallrna-5p, solid, poly-a, poly-g --, NAME=SEQ or a bare SEQ, which is its own
//               name.  N (default 5, capped at a probe's length) and PCT (default 10) hold for every probe.  The lines follow
//               the summary's: "probe", number, name, sequence, N, PCT, reads_with, bases_behind, reads_whole, reads_emptied;
//               the same for "any"; "probepos", probe, row, count for every non-zero cell.  --adapters with d, x or t or
//               without a report to write, an item that is neither a built-in name nor a valid adapter, more than 16 probes,
//               and --adapter with s or c are usage errors.  Without --adapters every output is what it was)
// (fqcomp28 c --i1 in.fastq -o out.fqc -t N / fqcomp28 d -i out.fqc --o1 out.fastq, src/app.cpp:29-76.)
// Prints one JSON line with sizes, seconds and blocks per worker; d and x also say how many blocks were decoded from a decode
// index ("index": "used") or were given one ("built"), and its bytes; "sums" / "verified" / "crc32": what became of the chunk
// sums file, the blocks whose digest was compared and held, the whole file's CRC-32; with --fasta also "form": "fasta" and the
// bytes read of the archive; with a report "stats": its path, "bases" and "mean_quality" (total Phred / bases, the one
// number that is no integer and in no report), with --adapters also "adapters", the number of probes, and "reads_with_any";
// with a filter "filter": what was read, what was kept and what each
// criterion dropped ("records" / "raw_bytes" of the line are then what was written); with a trim "trim": the same and the
// reads trimmed, the bases cut from either end and the reads emptied, and with an adapter -- then alone -- the reads in which it
// was found and the bases it took, and with a poly or window option -- then alone -- the reads with a poly tail, the bases it
// took, the reads the window cut and the bases it took.  With --mate the line's "records" / "raw_bytes" are mate 1's output,
// "raw_bytes2" mate 2's, "pairs": {"pairs", "kept", "dropped_mate1_only", "dropped_mate2_only", "dropped_both"} what became of
// the pairs, "blocks1" / "blocks2" the archives' chunks and "decodes2" the chunk decodes of archive 2, "sums2" / "verified2"
// (per decode) its chunk sums; with a selection option "mate1" and "mate2" replace "filter" and "trim": the keys of "trim", the
// adapter, poly and window keys always there, and "dropped_unmarked", the reads that passed and whose mate did not.  With
// an overlap option "overlap": {"pairs_overlapped", "pairs_read_through", "bases_behind_1", "bases_behind_2",
// "pairs_not_analysed"}; with --overlap-trim "mate1" / "mate2" are there and end in "reads_cut_limit", "bases_cut_limit"; with
// --overlap-correct, and only then, "overlap" ends in "pairs_corrected", "bases_corrected_1", "bases_corrected_2", "n_resolved".
// With --merge, and only then, "pairs" ends in "merged" (pairs = kept + merged + the three dropped counts) and the line has
// "merge": {"pairs_merged", "bases_merged", "bytes_merged", "overlap_bases", "places_disagree", "places_n", "pairs_too_short"}.
// Needs a GPU: no CPU fallback.
#include "../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace fqcomp28;

int main(int argc, char **argv) {
  const bool check_cmd = argc >= 2 && !strcmp(argv[1], "t");
  const bool index_cmd = argc >= 2 && !strcmp(argv[1], "x");
  const bool stats_cmd = argc >= 2 && !strcmp(argv[1], "s");
  const bool one_arg = index_cmd || check_cmd;  // x and t take the archive alone
  if (argc < (one_arg ? 3 : 4) || (strcmp(argv[1], "c") && strcmp(argv[1], "d") && !one_arg && !stats_cmd)) {
    std::fprintf(stderr, "usage: fqc_tool c|d <in> <out> [-t N] [-R MiB] [-S MiB] [-d 0,1,..] [--accumulate-n] [--index] [--index-stride KiSymbols] [--checksum] [--records A:B] [--stats report.tsv [--positions P]]\n"
                         "       fqc_tool d <in.fqc> <out.fastq> [-t N] [-d 0,1,..] [--min-len N] [--max-len N] [--max-n K] [--min-mean-q Q] [--max-low-q Q:PCT]\n"
                         "       fqc_tool d <in.fqc> <out.fastq> [-t N] [-d 0,1,..] [--cut-front N] [--cut-tail N] [--trim-q5 Q] [--trim-q3 Q] [--crop L] [filter options]\n"
                         "       fqc_tool d <in.fqc> <out.fastq> [-t N] [-d 0,1,..] --adapter SEQ [--adapter-overlap N] [--adapter-err PCT] [trim options] [filter options]\n"
                         "       fqc_tool d <in.fqc> <out.fastq> [-t N] [-d 0,1,..] [--poly-g [N] | --poly-x [N]] [--poly-every K] [--poly-mism M] [--window W:Q] [adapter options] [trim options] [filter options]\n"
                         "                  (the argument behind --poly-g / --poly-x is taken as N unless it begins with '-')\n"
                         "       fqc_tool d <in1.fqc> <out1.fastq> --mate <in2.fqc> <out2.fastq> [--adapter2 SEQ] [--overlap-trim] [--overlap-report file.tsv] [--overlap-min N] [--overlap-mism M] [--overlap-err PCT] [--overlap-correct] [--correct-q GOOD:BAD] [--merge merged.fastq] [--merge-min-len N] [--merge-floor-q Q] [-t N] [-d 0,1,..] [poly, window, adapter, trim and filter options]\n"
                         "                  (paired: a pair is kept only if both mates pass; the read ids of every pair are compared)\n"
                         "       fqc_tool d <in.fqc> <out.fasta> --fasta [-t N] [-d 0,1,..] [--records A:B]\n"
                         "       fqc_tool x <in.fqc> [-t N] [-d 0,1,..] [--index-stride KiSymbols]\n"
                         "       fqc_tool t <in.fqc> [-t N] [-d 0,1,..]\n"
                         "       fqc_tool s <in.fqc> <report.tsv> [-t N] [-d 0,1,..] [--positions P]\n"
                         "       fqc_tool s|c ... --adapters all|NAME|NAME=SEQ|SEQ,... [--adapter-overlap N] [--adapter-err PCT]   (c: with --stats)\n");
    return 2;
  }
  Settings set;
  bool range = false, fasta = false;
  std::string stats_path = stats_cmd ? argv[3] : "";
  bool stats_opt = false;
  long positions = -1;
  std::size_t rec_a = 0, rec_b = SIZE_MAX;
  fqgpu_filter filter = {0, FQGPU_FILTER_NONE, FQGPU_FILTER_NONE, 0, 0, 0, {0, 0}};
  bool filtered = false;
  fqgpu_trim trim = {0, 0, 0, 0, FQGPU_FILTER_NONE, {0, 0, 0}};
  bool trimmed = false;
  fqgpu_adapter adapter = {{0}, 0, 5, 10, 0};
  bool clipped = false, adapter_opt = false;
  fqgpu_adapter adapter2 = {{0}, 0, 5, 10, 0};
  bool clipped2 = false, mate = false;
  fqgpu_overlap overlap = {30, 5, 20, {0, 0, 0, 0, 0}};  // --overlap-min, --overlap-mism, --overlap-err
  bool overlap_opt = false, overlap_trim = false;       // one of the five options; --overlap-trim
  std::string overlap_path;                             // --overlap-report
  fqgpu_correct correct = {30, 14, {0, 0, 0, 0, 0, 0}};  // --correct-q
  bool overlap_correct = false, correct_opt = false;    // --overlap-correct; --correct-q
  fqgpu_merge merge = {2, 1, {0, 0, 0, 0, 0, 0}};        // --merge-floor-q, --merge-min-len
  std::string merge_path;                               // --merge
  bool merge_opt = false;                               // --merge-min-len or --merge-floor-q
  std::string mate_in, mate_out;
  std::string adapters_list;
  bool adapters_opt = false;
  fqgpu_tail tail = {0, 0, 0, 0, 0, 0, {0, 0}};
  uint32_t poly_every = 8, poly_mism = 5;
  bool tailed = false, poly_opt = false;
  // a decimal number of at most nine digits (so that it fits a uint32_t)
  const auto u32 = [](const std::string &t, uint32_t &out) {
    if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos) return false;
    out = static_cast<uint32_t>(std::stoul(t));
    return true;
  };
  for (int i = one_arg ? 3 : 4; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> const char * { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
    if (a == "-t") set.n_threads = (unsigned)std::atoi(val());
    else if (a == "-R") set.reading_chunk_size = (std::size_t)std::atoll(val()) << 20;
    else if (a == "-S") set.sample_chunk_size = (std::size_t)std::atoll(val()) << 20;
    else if (a == "--accumulate-n") set.accumulate_n_buffers = true;
    else if (a == "--fasta") fasta = true;
    else if (a == "--stats") { stats_opt = true; stats_path = val(); }
    else if (a == "--positions") positions = std::atol(val());
    else if (a == "--index" && !check_cmd && !stats_cmd) set.decode_index = true;  // (t builds nothing)
    else if (a == "--checksum" && argv[1][0] == 'c') set.checksum = true;
    else if (a == "--index-stride" && !check_cmd && !stats_cmd) { set.decode_index = true; set.index_stride = static_cast<unsigned>(std::atoi(val())) << 10; }  // Ki symbols
    else if (a == "--min-len" || a == "--max-len" || a == "--max-n" || a == "--min-mean-q") {
      const std::string v = val();
      uint32_t &field = a == "--min-len" ? filter.min_len : a == "--max-len" ? filter.max_len : a == "--max-n" ? filter.max_n : filter.min_mean_q;
      if (!u32(v, field)) {
        std::fprintf(stderr, "%s %s: expected a number\n", a.c_str(), v.c_str());
        return 2;
      }
      filtered = true;
    } else if (a == "--max-low-q") {
      const std::string v = val();
      const std::size_t colon = v.find(':');
      if (colon == std::string::npos || !u32(v.substr(0, colon), filter.low_q) || !u32(v.substr(colon + 1), filter.max_low_pct)) {
        std::fprintf(stderr, "--max-low-q %s: expected Q:PCT (at most PCT percent of a read's Phred values below Q)\n", v.c_str());
        return 2;
      }
      filtered = true;
    }
    else if (a == "--cut-front" || a == "--cut-tail" || a == "--trim-q5" || a == "--trim-q3" || a == "--crop") {
      const std::string v = val();
      uint32_t &field = a == "--cut-front" ? trim.cut_front : a == "--cut-tail" ? trim.cut_tail : a == "--trim-q5" ? trim.q_front
                        : a == "--trim-q3" ? trim.q_tail : trim.crop;
      if (!u32(v, field)) {
        std::fprintf(stderr, "%s %s: expected a number\n", a.c_str(), v.c_str());
        return 2;
      }
      trimmed = true;
    }
    else if (a == "--adapter") {
      const std::string v = val();
      adapter.len = static_cast<uint32_t>(v.size());  // (too long a one is refused by the check below)
      std::memset(adapter.seq, 0, sizeof adapter.seq);
      std::memcpy(adapter.seq, v.data(), std::min<std::size_t>(v.size(), FQGPU_ADAPTER_MAX));
      clipped = true;
    } else if (a == "--adapter2") {
      const std::string v = val();
      adapter2.len = static_cast<uint32_t>(v.size());  // (too long a one is refused by the check below)
      std::memset(adapter2.seq, 0, sizeof adapter2.seq);
      std::memcpy(adapter2.seq, v.data(), std::min<std::size_t>(v.size(), FQGPU_ADAPTER_MAX));
      clipped2 = true;
    } else if (a == "--mate") {
      mate_in = val();
      mate_out = val();
      mate = true;
    } else if (a == "--overlap-trim") {
      overlap_trim = overlap_opt = true;
    } else if (a == "--overlap-correct") {
      overlap_correct = overlap_opt = true;
    } else if (a == "--correct-q") {
      const std::string v = val();
      const std::size_t colon = v.find(':');
      if (colon == std::string::npos || !u32(v.substr(0, colon), correct.good_q) || !u32(v.substr(colon + 1), correct.bad_q)) {
        std::fprintf(stderr, "--correct-q %s: expected GOOD:BAD (two Phred values)\n", v.c_str());
        return 2;
      }
      correct_opt = true;
    } else if (a == "--merge") {
      merge_path = val();
      overlap_opt = true;
    } else if (a == "--merge-min-len" || a == "--merge-floor-q") {
      const std::string v = val();
      if (!u32(v, a == "--merge-min-len" ? merge.min_len : merge.floor_q)) {
        std::fprintf(stderr, "%s %s: expected a number\n", a.c_str(), v.c_str());
        return 2;
      }
      merge_opt = true;
    } else if (a == "--overlap-report") {
      overlap_path = val();
      overlap_opt = true;
    } else if (a == "--overlap-min" || a == "--overlap-mism" || a == "--overlap-err") {
      const std::string v = val();
      if (!u32(v, a == "--overlap-min" ? overlap.min_overlap : a == "--overlap-mism" ? overlap.max_mism : overlap.max_err_pct)) {
        std::fprintf(stderr, "%s %s: expected a number\n", a.c_str(), v.c_str());
        return 2;
      }
      overlap_opt = true;
    } else if (a == "--adapters") {
      adapters_list = val();
      adapters_opt = true;
    } else if (a == "--adapter-overlap" || a == "--adapter-err") {
      const std::string v = val();
      if (!u32(v, a == "--adapter-overlap" ? adapter.min_overlap : adapter.max_err_pct)) {
        std::fprintf(stderr, "%s %s: expected a number\n", a.c_str(), v.c_str());
        return 2;
      }
      adapter_opt = true;
    }
    else if (a == "--poly-g" || a == "--poly-x") {
      tail.poly_bases = a == "--poly-g" ? 4u : 15u;
      tail.poly_min_len = 10;
      if (i + 1 < argc && argv[i + 1][0] != '-') {  // [N]
        const std::string v = argv[++i];
        if (!u32(v, tail.poly_min_len)) {
          std::fprintf(stderr, "%s %s: expected a number\n", a.c_str(), v.c_str());
          return 2;
        }
      }
      tailed = true;
    } else if (a == "--poly-every" || a == "--poly-mism") {
      const std::string v = val();
      if (!u32(v, a == "--poly-every" ? poly_every : poly_mism)) {
        std::fprintf(stderr, "%s %s: expected a number\n", a.c_str(), v.c_str());
        return 2;
      }
      poly_opt = true;
    } else if (a == "--window") {
      const std::string v = val();
      const std::size_t colon = v.find(':');
      if (colon == std::string::npos || !u32(v.substr(0, colon), tail.window_len) || !u32(v.substr(colon + 1), tail.window_q) || !tail.window_len) {
        std::fprintf(stderr, "--window %s: expected W:Q (cut in the first window of W bases, 1 .. 32, whose mean Phred is below Q, 1 .. 64)\n", v.c_str());
        return 2;
      }
      tailed = true;
    }
    else if (a == "--records" && argv[1][0] == 'd') {
      // A:B or A: (decimal record numbers)
      const std::string v = val();
      const std::size_t colon = v.find(':');
      const auto number = [](const std::string &t, std::size_t &out) {
        if (t.empty() || t.size() > 19 || t.find_first_not_of("0123456789") != std::string::npos) return false;
        out = std::stoull(t);
        return true;
      };
      if (colon == std::string::npos || !number(v.substr(0, colon), rec_a) ||
          (colon + 1 < v.size() && !number(v.substr(colon + 1), rec_b))) {
        std::fprintf(stderr, "--records %s: expected A:B or A: (record numbers from 0)\n", v.c_str());
        return 2;
      }
      if (rec_a >= rec_b) {
        std::fprintf(stderr, "--records %s: an empty range\n", v.c_str());
        return 2;
      }
      range = true;
    } else if (a == "-d") {
      set.devices.clear();
      for (const char *p = val(); *p;) { set.devices.push_back(std::atoi(p)); while (*p && *p != ',') ++p; if (*p) ++p; }
    } else { std::fprintf(stderr, "unknown option %s\nusage: fqc_tool c|d <in> <out> [options] | fqc_tool x|t <in.fqc> [options]\n", a.c_str()); return 2; }
  }
  if (mate && (argv[1][0] != 'd' || range || fasta || set.decode_index)) {  // (said before any device is touched)
    std::fprintf(stderr, "--mate goes with a plain d alone: not with c, x, t, s, --records, --fasta, --index or --index-stride\n");
    return 2;
  }
  if (correct_opt && !overlap_correct) {
    std::fprintf(stderr, "--correct-q sets the two Phred values of --overlap-correct: it needs that option\n");
    return 2;
  }
  if (merge_opt && merge_path.empty()) {
    std::fprintf(stderr, "--merge-min-len and --merge-floor-q set the merge of --merge <merged.fastq>: they need that option\n");
    return 2;
  }
  if (overlap_opt && !mate) {
    std::fprintf(stderr, "--overlap-trim, --overlap-report, --overlap-correct, --merge, --overlap-min, --overlap-mism and --overlap-err analyse the two mates of a pair: they need --mate <in2.fqc> <out2.fastq>\n");
    return 2;
  }
  if (overlap_opt && !overlap_trim && !overlap_correct && overlap_path.empty() && merge_path.empty()) {
    std::fprintf(stderr, "--overlap-min, --overlap-mism and --overlap-err need --overlap-trim, --overlap-correct, --merge <merged.fastq> or --overlap-report <file.tsv>\n");
    return 2;
  }
  if (overlap_opt && fqgpu_overlap_check(&overlap) != FQGPU_OK) {
    std::fprintf(stderr, "mate overlap: expected --overlap-min 1 .. 512, --overlap-mism 0 .. 65535, --overlap-err 0 .. 50\n");
    return 2;
  }
  if (overlap_correct && fqgpu_correct_check(&correct) != FQGPU_OK) {
    std::fprintf(stderr, "overlap correction: expected --correct-q GOOD:BAD with GOOD 1 .. 63 and BAD below GOOD\n");
    return 2;
  }
  if (!merge_path.empty() && fqgpu_merge_check(&merge) != FQGPU_OK) {
    std::fprintf(stderr, "mate merging: expected --merge-min-len 1 .. 1023 and --merge-floor-q 0 .. 63\n");
    return 2;
  }
  if (!merge_path.empty() && (trim.cut_front || trim.cut_tail || trim.crop != FQGPU_FILTER_NONE)) {
    std::fprintf(stderr, "--merge does not go with --cut-front, --cut-tail or --crop: positional cuts have no defined meaning on a merged read yet\n");
    return 2;
  }
  if (clipped2 && !mate) {
    std::fprintf(stderr, "--adapter2 is mate 2's adapter: it needs --mate <in2.fqc> <out2.fastq>\n");
    return 2;
  }
  if (fasta && (argv[1][0] != 'd' || set.decode_index)) {  // (said before any device is touched)
    std::fprintf(stderr, "--fasta goes with d alone, and builds no index: not with c, x, t, --index or --index-stride\n");
    return 2;
  }
  if (filtered && (argv[1][0] != 'd' || range || fasta || set.decode_index)) {  // (said before any device is touched)
    std::fprintf(stderr, "a read filter goes with a plain d alone: not with c, x, t, s, --records, --fasta, --index or --index-stride\n");
    return 2;
  }
  if (filtered && fqgpu_filter_check(&filter) != FQGPU_OK) {
    std::fprintf(stderr, "the read filter: expected --min-len <= --max-len, --min-mean-q 0 .. 63, --max-low-q Q:PCT with Q 0 .. 64 and PCT 0 .. 100\n");
    return 2;
  }
  if (trimmed && (argv[1][0] != 'd' || range || fasta || set.decode_index)) {  // (said before any device is touched)
    std::fprintf(stderr, "read trimming goes with a plain d alone: not with c, x, t, s, --records, --fasta, --index or --index-stride\n");
    return 2;
  }
  if (trimmed && fqgpu_trim_check(&trim) != FQGPU_OK) {
    std::fprintf(stderr, "read trimming: expected --cut-front and --cut-tail 0 .. 65535, --trim-q5 and --trim-q3 0 .. 64, --crop 1 or more\n");
    return 2;
  }
  if (adapters_opt && ((argv[1][0] != 'c' && !stats_cmd) || stats_path.empty())) {  // (said before any device is touched)
    std::fprintf(stderr, "--adapters goes with s, and with c --stats <report.tsv>: not with d, x or t, and not without a report to write\n");
    return 2;
  }
  if (mate && !clipped2 && clipped) {  // (mate 2's adapter is mate 1's unless it has its own)
    std::memcpy(adapter2.seq, adapter.seq, sizeof adapter2.seq);
    adapter2.len = adapter.len;
  }
  if (mate) {  // (--adapter-overlap and --adapter-err hold for both)
    adapter2.min_overlap = adapter.min_overlap;
    adapter2.max_err_pct = adapter.max_err_pct;
    clipped2 = clipped2 || clipped;
  }
  if ((clipped || (adapter_opt && !adapters_opt)) && (argv[1][0] != 'd' || range || fasta || set.decode_index)) {  // (said before any device is touched)
    std::fprintf(stderr, "adapter clipping goes with a plain d alone: not with c, x, t, s, --records, --fasta, --index or --index-stride\n");
    return 2;
  }
  if (adapter_opt && !clipped && !clipped2 && !adapters_opt) {
    std::fprintf(stderr, "--adapter-overlap and --adapter-err need --adapter SEQ, or --adapters LIST\n");
    return 2;
  }
  fqgpu_probes probes = {};
  std::vector<std::string> probe_names;
  if (adapters_opt) {
    static const char *const builtin[][2] = {{"truseq", "AGATCGGAAGAGC"}, {"truseq-r1", "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"},
                                             {"truseq-r2", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"}, {"nextera", "CTGTCTCTTATACACATCT"},
                                             {"smallrna-3p", "TGGAATTCTCGG"}, {"smallrna-5p", "GATCGTCGGACT"}, {"solid", "CGCCTTGGCCGT"},
                                             {"poly-a", "AAAAAAAAAAAAAAAAAAAA"}, {"poly-g", "GGGGGGGGGGGGGGGGGGGG"}};
    // one probe more; false: it is no adapter fqgpu_adapter_check takes, or the seventeenth
    const auto add = [&](const std::string &name, const std::string &seq) {
      if (probes.n >= FQGPU_PROBES_MAX) {
        std::fprintf(stderr, "--adapters %s: more than %d probes\n", adapters_list.c_str(), FQGPU_PROBES_MAX);
        return false;
      }
      fqgpu_adapter p = {{0}, static_cast<uint32_t>(seq.size()), adapter.min_overlap, adapter.max_err_pct, 0};
      std::memcpy(p.seq, seq.data(), std::min<std::size_t>(seq.size(), FQGPU_ADAPTER_MAX));
      if (p.min_overlap > p.len) p.min_overlap = p.len;  // (N is capped at the probe's length, as d --adapter caps it)
      if (fqgpu_adapter_check(&p) != FQGPU_OK) {
        std::fprintf(stderr, "--adapters: %s is neither all, a built-in name nor 1 .. 64 bases ACGT (upper case); --adapter-overlap 1 or more, --adapter-err 0 .. 50\n",
                     name.c_str());
        return false;
      }
      probes.probe[probes.n++] = p;
      probe_names.push_back(name);
      return true;
    };
    for (std::size_t at = 0; at <= adapters_list.size();) {
      const std::size_t comma = std::min(adapters_list.find(',', at), adapters_list.size());
      const std::string item = adapters_list.substr(at, comma - at);
      at = comma + 1;
      const std::size_t eq = item.find('=');
      bool ok = true, known = false;
      if (item == "all") {
        for (const auto &b : builtin) ok = ok && add(b[0], b[1]);
        known = true;
      }
      for (const auto &b : builtin)
        if (item == b[0]) { ok = add(b[0], b[1]); known = true; }
      if (!known) ok = eq == std::string::npos ? add(item, item) : eq != 0 && add(item.substr(0, eq), item.substr(eq + 1));
      if (!ok) {
        if (eq == 0) std::fprintf(stderr, "--adapters: %s has no name in front of its =\n", item.c_str());
        return 2;
      }
    }
    set.probes = probes;
  }
  if (clipped) {
    if (adapter.min_overlap > adapter.len) adapter.min_overlap = adapter.len;  // (N is capped at the adapter's length)
    if (fqgpu_adapter_check(&adapter) != FQGPU_OK) {
      std::fprintf(stderr, "adapter clipping: expected --adapter of 1 .. 64 bases ACGT (upper case), --adapter-overlap 1 or more, --adapter-err 0 .. 50\n");
      return 2;
    }
  }
  if (clipped2) {
    if (adapter2.min_overlap > adapter2.len) adapter2.min_overlap = adapter2.len;  // (N is capped at the adapter's length)
    if (fqgpu_adapter_check(&adapter2) != FQGPU_OK) {
      std::fprintf(stderr, "adapter clipping: expected --adapter2 of 1 .. 64 bases ACGT (upper case), --adapter-overlap 1 or more, --adapter-err 0 .. 50\n");
      return 2;
    }
  }
  if ((tailed || poly_opt) && (argv[1][0] != 'd' || range || fasta || set.decode_index)) {  // (said before any device is touched)
    std::fprintf(stderr, "poly tails and the window cut go with a plain d alone: not with c, x, t, s, --records, --fasta, --index or --index-stride\n");
    return 2;
  }
  if (poly_opt && !tail.poly_bases) {
    std::fprintf(stderr, "--poly-every and --poly-mism need --poly-g or --poly-x\n");
    return 2;
  }
  if (tailed) {
    if (tail.poly_bases) {
      tail.poly_every = poly_every;
      tail.poly_max_mism = poly_mism;
    }
    if (fqgpu_tail_check(&tail) != FQGPU_OK) {
      std::fprintf(stderr, "tail trims: expected --poly-g / --poly-x 1 .. 65535, --poly-every 2 .. 255, --poly-mism 0 .. 255, --window W:Q with W 1 .. 32 and Q 1 .. 64\n");
      return 2;
    }
  }
  // (said before any device is touched)
  if (stats_opt && argv[1][0] != 'c') {
    std::fprintf(stderr, "--stats goes with c alone (s <in.fqc> <report.tsv> summarises an archive): not with d, x, t or s\n");
    return 2;
  }
  if (positions != -1 && stats_path.empty()) {
    std::fprintf(stderr, "--positions needs a report to write: c --stats <report.tsv>, or s\n");
    return 2;
  }
  if (positions != -1 && (positions < 1 || positions > 65535)) {
    std::fprintf(stderr, "--positions %ld: expected 1 .. 65535\n", positions);
    return 2;
  }
  if (!stats_path.empty()) set.stats_positions = positions == -1 ? 512u : static_cast<unsigned>(positions);
  try {
    const bool comp = argv[1][0] == 'c';
    if (!comp) {  // --index on the way back: build, not write
      set.build_index = set.decode_index && !range;
      set.decode_index = false;
    }
    const Selection sel{clipped ? &adapter : nullptr, tailed ? &tail : nullptr, trimmed ? &trim : nullptr, filtered ? &filter : nullptr,
                        overlap_opt ? &overlap : nullptr, overlap_trim, overlap_correct ? &correct : nullptr,
                        merge_path.empty() ? nullptr : &merge};
    PairedReport paired;
    if (mate) paired = processArchivePaired(argv[2], argv[3], mate_in, mate_out, clipped2 ? &adapter2 : nullptr, sel, set, merge_path);
    const FarmReport r = mate ? paired.mate1
                         : check_cmd || stats_cmd ? processArchiveCheck(argv[2], set)
                         : index_cmd ? processArchiveIndex(argv[2], set)
                         : comp    ? processReads(argv[2], argv[3], set)
                         : sel.trims() || filtered ? processArchiveSelected(argv[2], argv[3], sel, set)
                         : fasta   ? processArchiveFasta(argv[2], argv[3], rec_a, rec_b, set)
                         : range   ? processArchiveRange(argv[2], argv[3], rec_a, rec_b, set)
                                   : processArchiveParts(argv[2], argv[3], set);
    if (!overlap_path.empty()) writeOverlapReport(overlap_path, paired.overlap, overlap, sel.correct, paired.correct, sel.merge, paired.merge);
    if (!stats_path.empty() && adapters_opt) writeStatsReport(stats_path, r.stats, r.probes, probes, probe_names);
    else if (!stats_path.empty()) writeStatsReport(stats_path, r.stats);
    std::printf("{\"cmd\": \"%s\", \"threads\": %u, \"devices\": %zu, \"raw_bytes\": %zu, \"records\": %zu, \"blocks\": %zu, "
                "\"seq_bytes\": %zu, \"qual_bytes\": %zu, \"misc_bytes\": %zu, \"seconds\": %.6f, \"blocks_per_worker\": [",
                argv[1], set.n_threads, set.devices.size(), r.in.raw, r.in.n_records, comp ? r.out.n_blocks : (std::size_t)0,
                r.out.seq, r.out.qual, r.out.misc, r.seconds);
    for (std::size_t i = 0; i < r.blocks_per_worker.size(); ++i) std::printf("%s%u", i ? ", " : "", r.blocks_per_worker[i]);
    std::printf("]");
    if (!comp)
      std::printf(", \"index\": \"%s\", \"indexed_blocks\": %zu, \"index_bytes\": %zu", r.index_built ? "built" : r.indexed_blocks ? "used" : "none",
                  r.indexed_blocks, r.index_bytes);
    if (comp && set.checksum) std::printf(", \"sums\": \"%s\", \"crc32\": \"%08x\"", r.sums, r.file_crc32);
    if (!comp && argv[1][0] != 'x') {
      std::printf(", \"sums\": \"%s\", \"verified\": %zu", r.sums, r.verified_blocks);
      if (r.verified_blocks) std::printf(", \"crc32\": \"%08x\"", r.file_crc32);
    }
    if (!stats_path.empty()) {  // ("records" above is the summary's count as well)
      std::string quoted;
      for (const char ch : stats_path) { if (ch == '"' || ch == '\\') quoted += '\\'; quoted += ch; }
      std::printf(", \"stats\": \"%s\", \"bases\": %llu, \"mean_quality\": %.6f", quoted.c_str(), (unsigned long long)r.stats[1], statsMeanQuality(r.stats));
      if (adapters_opt)
        std::printf(", \"adapters\": %u, \"reads_with_any\": %llu", probes.n,
                    (unsigned long long)(r.probes.empty() ? 0 : r.probes[8 + probes.n * (8 + (std::size_t)set.stats_positions + 1)]));
    }
    if (mate) {
      std::printf(", \"raw_bytes2\": %zu, \"pairs\": {\"pairs\": %llu, \"kept\": %llu, \"dropped_mate1_only\": %llu, \"dropped_mate2_only\": %llu, "
                  "\"dropped_both\": %llu%s}, \"blocks1\": %zu, \"blocks2\": %zu, \"decodes2\": %zu, \"index2\": \"%s\", \"sums2\": \"%s\", \"verified2\": %zu",
                  paired.mate2.in.raw, (unsigned long long)paired.pairs, (unsigned long long)paired.kept, (unsigned long long)paired.dropped_mate1_only,
                  (unsigned long long)paired.dropped_mate2_only, (unsigned long long)paired.dropped_both,
                  sel.merge ? (", \"merged\": " + std::to_string(paired.merged)).c_str() : "", paired.blocks1, paired.blocks2, paired.decodes2,
                  paired.mate2.indexed_blocks ? "used" : "none", paired.mate2.sums, paired.mate2.verified_blocks);
      if (overlap_opt) {
        const auto w = [&](unsigned i) { return (unsigned long long)paired.overlap[i]; };
        std::printf(", \"overlap\": {\"pairs_overlapped\": %llu, \"pairs_read_through\": %llu, \"bases_behind_1\": %llu, \"bases_behind_2\": %llu, "
                    "\"pairs_not_analysed\": %llu", w(1), w(2), w(3), w(4), w(5));
        if (overlap_correct) {
          const auto c = [&](unsigned i) { return (unsigned long long)paired.correct[i]; };
          std::printf(", \"pairs_corrected\": %llu, \"bases_corrected_1\": %llu, \"bases_corrected_2\": %llu, \"n_resolved\": %llu", c(2), c(3), c(4), c(5));
        }
        std::printf("}");
      }
      if (sel.merge) {
        const auto g = [&](unsigned i) { return (unsigned long long)paired.merge[i]; };
        std::printf(", \"merge\": {\"pairs_merged\": %llu, \"bases_merged\": %llu, \"bytes_merged\": %llu, \"overlap_bases\": %llu, "
                    "\"places_disagree\": %llu, \"places_n\": %llu, \"pairs_too_short\": %llu}", g(2), g(3), g(4), g(5), g(6), g(7), g(11));
      }
      for (int m = 0; m < 2 && (filtered || trimmed || clipped || clipped2 || tailed || overlap_trim); ++m) {
        const std::vector<uint64_t> &t = m ? paired.mate2.trim : paired.mate1.trim;
        const auto w = [&](unsigned i) { return (unsigned long long)t[i]; };
        std::printf(", \"mate%d\": {\"records\": %llu, \"kept\": %llu, \"bases_in\": %llu, \"bases_kept\": %llu, \"bytes_kept\": %llu, "
                    "\"dropped_short\": %llu, \"dropped_long\": %llu, \"dropped_n\": %llu, \"dropped_mean_q\": %llu, \"dropped_low_q\": %llu, "
                    "\"reads_trimmed\": %llu, \"bases_cut_front\": %llu, \"bases_cut_tail\": %llu, \"reads_emptied\": %llu, "
                    "\"reads_with_adapter\": %llu, \"bases_cut_adapter\": %llu, \"reads_with_poly_tail\": %llu, \"bases_cut_poly\": %llu, "
                    "\"reads_window_cut\": %llu, \"bases_cut_window\": %llu, \"dropped_unmarked\": %llu",
                    m + 1, w(0), w(1), w(2), w(3), w(4), w(5), w(6), w(7), w(8), w(9), w(10), w(11), w(12), w(13), w(14), w(15), w(16), w(17), w(18),
                    w(19), w(20));
        if (overlap_trim) std::printf(", \"reads_cut_limit\": %llu, \"bases_cut_limit\": %llu", w(21), w(22));
        std::printf("}");
      }
    }
    if (filtered && !mate) {
      const auto w = [&](unsigned i) { return (unsigned long long)(sel.trims() ? r.trim[i] : r.filter[i]); };  // (words 0 .. 9 are the same)
      std::printf(", \"filter\": {\"records\": %llu, \"kept\": %llu, \"bases_in\": %llu, \"bases_kept\": %llu, \"dropped_short\": %llu, "
                  "\"dropped_long\": %llu, \"dropped_n\": %llu, \"dropped_mean_q\": %llu, \"dropped_low_q\": %llu}",
                  w(0), w(1), w(2), w(3), w(5), w(6), w(7), w(8), w(9));
    }
    if (sel.trims() && !mate) {
      const auto w = [&](unsigned i) { return (unsigned long long)r.trim[i]; };
      std::printf(", \"trim\": {\"records\": %llu, \"kept\": %llu, \"bases_in\": %llu, \"bases_kept\": %llu, \"bytes_kept\": %llu, "
                  "\"dropped_short\": %llu, \"dropped_long\": %llu, \"dropped_n\": %llu, \"dropped_mean_q\": %llu, \"dropped_low_q\": %llu, "
                  "\"reads_trimmed\": %llu, \"bases_cut_front\": %llu, \"bases_cut_tail\": %llu, \"reads_emptied\": %llu",
                  w(0), w(1), w(2), w(3), w(4), w(5), w(6), w(7), w(8), w(9), w(10), w(11), w(12), w(13));
      if (clipped) std::printf(", \"reads_with_adapter\": %llu, \"bases_cut_adapter\": %llu", w(14), w(15));
      if (tailed)
        std::printf(", \"reads_with_poly_tail\": %llu, \"bases_cut_poly\": %llu, \"reads_window_cut\": %llu, \"bases_cut_window\": %llu", w(16), w(17),
                    w(18), w(19));
      std::printf("}");
    }
    if (fasta) std::printf(", \"form\": \"fasta\", \"archive_bytes_read\": %llu", (unsigned long long)r.archive_bytes_read);
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "fqc_tool: %s\n", e.what());
    return 1;
  }
  return 0;
}
