#!/usr/bin/env python3
"""Rewrite the "## Round 6" section of profiles/README.md from the committed round-6 files (so that the section's numbers are
the files' numbers):   python tools/gen_profiles_readme_r06.py"""
import csv
import json
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
P = ROOT / "profiles"
c = json.loads((P / "fragani_counters.json").read_text())
w = c["map_segments_kernel"]["work"]
ph = w["valu_instructions_per_phase_per_segment"]
u = w["algorithmic_units_per_dispatch"]
parts = w["algorithmic_valu_instructions_by_unit"]
bh, sp, mi, ms = c["bucket_hits_kernel"], c["map_sparse_kernel"], c["minimizer_kernel"], c["map_segments_kernel"]
bench = json.loads((P / "r06_bench_n1000_result.json").read_text().strip().splitlines()[-1])
fa, fr, cf = bench["also"]["fragment_ani"], bench["also"]["fragment_ani_rearranged"], bench["config1_files"]
goc = bench["cpu_baseline"]["gpu_over_cpu"]
ws = fa["workspace_device_bytes"]
stats = {}
with (P / "r06_fragani_n1000_kernel_stats.csv").open() as fh:
    for r in csv.DictReader(fh):
        stats[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]) / 1e6, float(r["TotalDurationNs"]) / 1e6)


def kern(pattern):
    for name, v in stats.items():
        if pattern in name:
            return v
    return (0, float("nan"), float("nan"))


cuts_t = {}
for line in (P / "r06_map_segments_phase_cuts.txt").read_text().splitlines():
    m = re.match(r"cut (\d+): frag_map\s+(\S+) ms\s+\(\+\s*(\S+)\)", line)
    if m:
        cuts_t.setdefault(int(m.group(1)), (float(m.group(2)), float(m.group(3))))
rear = json.loads((P / "fragani_rearranged_events.json").read_text())
ev_r, ev_s = rear["rearranged"], rear["substitution_only"]
pm = lambda x: f"{x:.0f}"  # noqa: E731

text = f'''## Round 6

All files of this round are from the final build (`tools/profile_round.sh r06`).  **No scaling curve has been measured in this round either** (one-GPU
boxes); what ran on hardware at world 8 is the plumbing: `tests/test_gpu_00_multi_gpu_path.py` (eight ranks of `bench.py --gpus 8` and of both product
drivers sharing the one device, gloo).

| file | what |
|---|---|
| `r06_bench_n1000_result.json` | the JSON line of an un-profiled `python bench.py --full --steps 20 --warmup 5`: `value` {bench["value"]:.3g} pairs/s ({bench["ms_per_step"]:.2f} ms), `cpu_baseline.gpu_over_cpu` (T_e2e strict {goc["t_e2e_strict_pairs_per_s"]:.3g} pairs/s = {goc["t_e2e_strict_over_cpu"]:.0f} x the CPU port; `value` {goc["value_over_cpu"]:.0f} x), `also.fragment_ani` {fa["seconds_per_run"]:.3f} s per 10^6 pairs (index {fa["phases_ms_per_run"]["frag_index"]:.0f} ms, seeding {fa["phases_ms_per_run"]["frag_seed"]:.0f}, mapping {fa["phases_ms_per_run"]["frag_map"]:.0f}), `workspace_device_bytes` ({ws["all_columns"]["held_bytes"] / 1e9:.1f} / {ws["one_eighth_of_the_columns"]["held_bytes"] / 1e9:.1f} / {ws["one_column"]["held_bytes"] / 1e9:.1f} GB for all columns / an eighth / one), `also.fragment_ani_rearranged` {fr["seconds_per_run"]:.3f} s, `config1_files` (T_file {cf["seconds"]:.3f} s, matrices {cf["matrices"]}) as the line's last key |
| `r06_bench_n1000_kernel_stats.csv`, `hash_counters.json`, `r06_pmc_kmer_hash_summary.txt` | the headline step's kernels: `kmer_hash_kernel<31,true>` 11.3 ms, 92.4 vector instructions per wave-window, VALUBusy 106 %, traffic 1.38 GB per launch (1.07 x algorithmic): unchanged, untouched |
| `r06_fragani_n1000_kernel_stats.csv` | `rocprofv3 --kernel-trace --stats -- python3 tools/bench_fragani.py 1000 0`: `minimizer_kernel<16>` **{kern("minimizer_kernel<16>")[1]:.1f} ms** (44.0 in round 5), `postings_kernel` {kern("postings_kernel")[1]:.1f} (19.3), `rs_scatter` 4 x {kern("rs_scatter_kernel")[1]:.1f}, `map_segments_kernel<320u, true>` {kern("map_segments_kernel<320u, true>")[2] / 2:.0f} ms per run, `map_sparse_kernel` {kern("map_sparse_kernel")[2] / 2:.0f}, `bucket_hits_staged_kernel` {kern("bucket_hits_staged_kernel")[2] / 2:.0f} |
| `r06_pmc_minimizer_summary.txt`, `r06_pmc_postings_summary.txt`, `r06_pmc_rs_scatter_summary.txt` | counter passes of the index kernels (the round-5 verdict's missing evidence).  Minimizer: {mi["valu_instructions"]:.4g} vector instructions = **{mi["valu_instructions_per_position"]:.0f} per position** (263 before the hash-only winnowing), VALUBusy {mi["valu_busy"]:.2f}, {mi["waves_per_simd"]:.1f} waves per SIMD, {100 * mi["wait_share"]:.0f} % of wave time waiting; before the per-XCD tickets and the per-tile contig table the same instruction stream took 47 ms at VALUBusy 0.55 (a tile lived ~24 us of which it computed 3).  Postings: the scatter of the hash ids into position order (4-byte stores, a sector each; WRITE_SIZE 17 GB counted for 4*10^8 postings) is what it waits for (96 % of wave time).  `rs_scatter`: 3.6 ms per pass of 4*10^8 (key, value) pairs = 9.6 GB moved per pass = 2.6 TB/s |
| `r06_pmc_map_segments_summary.txt`, `r06_pmc_map_sparse_summary.txt`, `r06_pmc_bucket_hits_summary.txt` | counter passes of the mapping and seeding kernels at the benchmarked size (one batch of 2^17 fragments).  General kernel: **{ms["avg_ms_per_dispatch"]:.1f} ms** per dispatch of 2.90 million segments (25.1), {ms["valu_instructions"]:.4g} vector instructions = **{ms["valu_instructions_per_segment"]:.0f} per segment** (4 100), VALUBusy {ms["valu_busy"]:.2f}, {100 * ms["wait_share"]:.0f} % of wave time waiting, {ms["waves_per_simd"]:.1f} waves per SIMD.  Sparse kernel: {sp["avg_ms_per_dispatch"]:.2f} ms per dispatch of {sp["segments_per_dispatch"]:.0f} segments, VALUBusy {sp["valu_busy"]:.2f}.  Seeding: {bh["avg_ms_per_dispatch"]:.2f} ms per dispatch of {bh["seed_hits_per_dispatch"]:.3g} seed hits |
| `r06_map_cut_valu.txt` | `tools/map_cut_valu.sh`: **the instruction counter per phase** the round-5 verdict asked for -- `SQ_INSTS_VALU` (and SALU, LDS) of the general kernel cut short after each phase (tools build, `enum MapCut`), same batch.  `r06_map_cut_valu_start_of_round.txt`: the same at the start of the round (every segment's hits through the bitonic network: 625 vector instructions per segment for ordering and staging; {pm(ph["hits_ordered_and_staged"])} now) |
| `r06_map_segments_phase_cuts.txt` | `tools/map_cut.py`: the same cuts timed (ms per 1 000-genome run, tools build; every line holds the sparse kernel's ~57 ms): record + sketch {cuts_t[10][0] - 57:.0f}, hits ordered and staged **{cuts_t[11][1]:.0f}** (28 in round 5), bucket table {cuts_t[1][1]:.0f}, L1 {cuts_t[2][1]:.0f}, candidate set-up {cuts_t[3][1]:.0f}, seed-hit bounds {cuts_t[4][1]:.0f} (upper estimate), first group only {cuts_t[23][0]:.0f} of {cuts_t[9][0]:.0f} |
| `r06_fragani_n1000_one_batch_trace.txt`, `r06_fragani_n1000_rearranged_one_batch_trace.txt`, `fragani_rearranged_events.json` | `tools/map_stats.py 1000 78` (stats build; `PA_SYNTH=rearranged` for the second): event counts of the mapping kernels, now with the layout of a segment's hits (one cluster: {100 * ev_s["share_hits_one_cluster"]:.0f} / {100 * ev_r["share_hits_one_cluster"]:.0f} %; plus one stray: {100 * ev_s["share_one_cluster_but_one_hit"]:.0f} / {100 * ev_r["share_one_cluster_but_one_hit"]:.0f} %; plus two: {100 * ev_s["share_one_cluster_but_two_hits"]:.0f} / {100 * ev_r["share_one_cluster_but_two_hits"]:.0f} %), the segments that skip the L1 scan ({100 * ev_s["share_of_one_run_segments_no_l1_scan"]:.0f} / {100 * ev_r["share_of_one_run_segments_no_l1_scan"]:.0f} %), candidates per segment ({ev_s["candidates_per_segment"]:.2f} / {ev_r["candidates_per_segment"]:.2f}), rounds per segment ({ev_s["rounds_per_segment"]:.2f} / {ev_r["rounds_per_segment"]:.2f}), and the sparse kernel's counters (groups, begins, states, ties) |
| `r06_fragani_n1000_rearranged_run.txt` | `PA_SYNTH=rearranged python3 tools/bench_fragani.py 1000`: the whole run on the set with indels, rearrangements, repeat families and contigs |
| `r06_fetch_calibration.txt` | `tools/fetch_calib.sh`: what `FETCH_SIZE` counts for the seeding kernel's access pattern (`tools/fetch_calib.hip`: 24 million runs of ~18 items at unrelated places of a 2 GiB array, eight lists per lane in flight, the host knowing every byte asked for and every 64-byte line touched): wide streaming reads 0.500 of the bytes (the guide's rule, reproduced in the same run); runs of 2-byte items {bh["fetch_calibration"]["counted_over_asked_2_byte_runs"]:.3f} x the bytes asked = {bh["fetch_calibration"]["counted_over_line_bytes_2_byte_runs"]:.3f} of the 64-byte lines touched; runs of 8-byte items {bh["fetch_calibration"]["counted_over_asked_8_byte_runs"]:.3f} x the bytes asked = {bh["fetch_calibration"]["counted_over_line_bytes_8_byte_runs"]:.3f} of the lines |
| `r06_variants_agree.txt`, `r06_fragani_stress.txt` | `tools/variants_agree.sh`: the product build and five compile-time variants (every segment through the L1 scan; no bound at a round's end; rounds of two passes; every segment's hits through the network; no L1 skip for runs with strays) on the benchmark's 10^6 pairs: one sha256 over every result, identical (38 200 184 kept fragments -- as at the start of the round and in every build of round 5).  `tests/tools/fragani_stress.py`: 450 random sets + 8 Mb-sized sets with the frequency cut active, device against oracle, no difference |
| `fragani_counters.json` | `python tools/pmc_fragani_to_json.py r06`: everything `bench.py` copies into `also.fragment_ani.roofline`, `.roofline_sparse`, `.roofline_index`, `.roofline_seeding`; `tests/test_host_logic.py::test_work_based_roofline_is_reproducible_from_the_committed_profiles` rebuilds it from the files above and re-derives every fraction by hand |

### Work-based roofline of the mapping kernel, round 6 (`also.fragment_ani.roofline`): every number measured

`frac` = vector instructions the dispatch NEEDS with a perfect bound / vector instructions it ISSUED.  Round 5 priced the units from a static
listing and charged the L1 scan to every hit (0.70; the verdict recomputed 0.59).  Now every price is a difference of two measured counts -- the
kernel cut short after a phase under `--pmc SQ_INSTS_VALU` -- so what a segment does not do is not charged:

| phase (cut) | vector instructions per segment |
|---|---|
| record and sketch (10) | {pm(ph["record_and_sketch"])} |
| hits ordered and staged (11) | {pm(ph["hits_ordered_and_staged"])} (625 with every segment through the network) |
| sketch table (1) | {pm(ph["sketch_table"])} |
| L1: the run test, the scan where one is needed, the candidate handed over (2) | {pm(ph["l1"])} |
| candidate set-up (3) | {pm(ph["candidate_set_up"])} |
| first round: group bound, stretch, window ends, tight bound, ranks, match bitmap (5) | {pm(ph["first_round_bound_stretch_ranks_bitmap"])} |
| ... items and coarse table (7) | {pm(ph["first_round_items_and_coarse_table"])} |
| ... window masks and coarse search (8) | {pm(ph["first_round_window_masks_and_coarse_search"])} |
| ... fine passes and fold: the first round complete (24) | {pm(ph["first_round_fine_passes_and_fold"])} |
| the rest of the first group (23) | {pm(ph["rest_of_the_first_group"])} |
| the other groups (9: the whole kernel) | {pm(ph["other_groups"])} |
| **whole kernel** | **{pm(ph["whole_kernel"])}** |

Needed: everything up to the candidate's set-up as issued, V[3] = {parts["fixed_up_to_the_candidates_set_up"]:.4g}; plus per candidate ONE complete round on the group of the expected optimum,
V[24] - V[3] = {(parts["one_round_per_candidate_share_of_one_window_and_the_ties"] / w["share_of_a_round_needed"]):.4g}, of which a perfect bound needs the share that one window's minimizers (237) and the further tying states
({u["tying_states"] / u["candidates"]:.2f} per candidate) are of the {w["entries_ranked_per_full_round"]:.1f} entries such a round ranks: share = {w["share_of_a_round_needed"]:.4f}.
needed = {parts["fixed_up_to_the_candidates_set_up"]:.4g} + {(parts["one_round_per_candidate_share_of_one_window_and_the_ties"] / w["share_of_a_round_needed"]):.4g} x {w["share_of_a_round_needed"]:.4f} = **{w["algorithmic_valu_instructions_per_dispatch"]:.4g}** of {w["counted_valu_instructions_per_dispatch"]:.4g} issued -> **frac = {w["frac"]:.3f}**.
`frac_first_group` = V[23] / V[9] = **{w["frac_first_group"]:.3f}**: what the kernel issues when it only ever looks at the 64 begins around the expected optimum (a perfect bound on whole groups), measured directly.
`frac_minimal_sort` = {w["frac_minimal_sort"]:.3f}: the same as `frac` with EVERY segment's hits ordered at the counting sort's price ({w["counting_sort_valu_per_segment"]:.0f} per segment, from the mix:
the network's {w["network_sort_valu_per_segment"]:.0f} is the start-of-round measurement) -- 96 % of the segments are counted already, so the two agree.
What is not algorithmic: the other groups of a candidate (a light round each: a stretch loaded, the tight bound asked, nothing ranked) and the rest of
the first group -- {ph["other_groups"] + ph["rest_of_the_first_group"]:.0f} of {ph["whole_kernel"]:.0f} instructions per segment --, and the part of the first round's entries beyond one window.
The product build's own counter pass ({ms["valu_instructions"]:.4g}) sits 2 % below the tools build's uncut run (the cut tests).

Other kernels of the path (`fragani_counters.json`):

* `map_sparse_kernel` (`roofline_sparse`): VALUBusy {sp["valu_busy"]:.2f} -- instructions are time --, {sp["valu_instructions_per_segment"]:.0f} vector instructions per segment = {sp["valu_instructions_per_state_evaluated"]:.2f} per state evaluated ({sp["events_per_dispatch"]["states"]:.4g} states of {sp["events_per_dispatch"]["begins"]:.4g} begins in {sp["events_per_dispatch"]["groups"]:.4g} groups per dispatch).  Work-based `frac` = groups that hold a candidate's first or last tying begin / groups evaluated = **{sp["frac"]:.2f}** ({sp["groups_per_segment"]:.1f} groups per segment, 3.9 at the start of the round): with two to eight hits nearly every window that holds them ties, and of the ties only the first and the last decide the position -- the kernel now starts at the first hit's group and leaves out the begins between two known ties unless they hold more hits than those share.  What is left: in two candidates of three one of the hits is shared by no window (its hash lies too high in the union), so the begins that hold every hit could share more by the count of their hits and are all evaluated; ruling them out needs the hit's count over every window, which is the evaluation.
* `minimizer_kernel<16>` (`roofline_index`): {mi["valu_instructions_per_position"]:.0f} vector instructions per position of which the two MurmurHash3 are 126 (the kernel's own hashing loop) -> `frac` **{mi["frac"]:.2f}**, VALUBusy {mi["valu_busy"]:.2f}; 0.2 TB/s of algorithmic bytes: not an HBM kernel.
* `bucket_hits_staged_kernel` (`roofline_seeding`): 18 algorithmic bytes per hit / {bh["avg_ms_per_dispatch"]:.2f} ms = {bh["algorithmic_gbs"] / 1000:.2f} TB/s = **{bh["algorithmic_gbs"] / 8000:.3f} of the HBM roof**; traffic: FETCH_SIZE {bh["fetch_bytes_per_hit_as_counted"]:.1f} counted bytes per hit x {bh["fetch_calibration"]["line_bytes_per_counted_byte"]:.3f} (the calibration's lines per counted byte for this mix of 2- and 8-byte runs) = {bh["fetch_bytes_per_hit_calibrated"]:.1f} + WRITE_SIZE {bh["write_bytes_per_hit"]:.1f} = **{bh["counter_bytes_per_hit"]:.1f} bytes per hit = {bh["traffic_over_algorithmic"]:.2f} x algorithmic** -- one calibrated number where round 5 gave two (1.13 x as counted, 1.81 x doubled).  The excess is the lines' unused halves: a run of eighteen 2-byte genomes is 36 bytes in a 64-byte line.

### Tried and withdrawn in round 6 (A/B on one box each, `tools/ab_fragani.sh` / `tools/ab_kernel.sh`)

* waves that go through many segments each instead of one workgroup per segment (no launch per segment, the next record within reach): the loop keeps
  the kernel's arguments and the scan state alive, 15 vector registers spilled: mapping 430 / 420 ms (one / four workgroups per wave slot) against 368;
* the seeding's counting pass over the 8-byte postings (so that the scatter pass finds them in the caches) instead of their 2-byte genomes: seeding 70 ms against 63.5;
* `minimizer_kernel` with 512 / 1 024 threads (half / a quarter of the tickets): 39.3 / 43.7 ms against 39.9 before the per-XCD counters -- the tile's life is waits, not the
  counter's throughput; all eight k-mers of a thread hashed side by side (102 registers, 4 waves per SIMD): 46.8 ms against 39.9 for four at a time (80 registers);
* the last L1 turn's one candidate handed to the evaluation straight from the scan's registers instead of through the list and the parked state in LDS: 126 -> 128
  registers, four spilled, mapping 364 ms against 359;
* the groups of begins next to the optimum's asked the tight bound against the stretch the group before has left in LDS (its entries below the pivot hash kept as
  bits), before they load a stretch of their own: the kept stretch holds 75-100 % of such a begin's narrowest window and the bound needs nearly all of it -- 31 of
  106 million begins dropped, 0.80 of 3.51 million groups ended there (rounds 6.85 -> 5.93 million per batch), the other groups pay the test twice: mapping 373 ms against 353;
* in the group of the expected optimum, a first round that takes the 64 states AROUND the optimum instead of the first 64 in slide order (so that the begins
  left over are as far from it as can be on both sides): 11.76 ms per dispatch against 11.48 -- the left-overs on the left were evaluated for free before;
* what the phase cuts promised and the A/Bs gave: ordering by counting, cluster alone: -5.5 ms of mapping (cut: 14 of 28); with strays -7.5 more; the L1 scan skipped for a run
  with strays: -1.4 (the cut's L1 phase is 21 ms, most of it the candidate's hand-over through LDS, which stays); in the sparse kernel the hits marked by position and one
  comparison per entry and hit instead of three: 3.39 -> 3.28 ms per batch, the end of a begin's last window taken from the next begin's search and the hit's
  allowance computed once per begin instead of once per pair of states: 3.30 -> 3.16, the one lane's own search done by the wave: -> 3.06, and the groups of
  begins between two tying begins left out (only the first and the last tying state count): -> 2.78, the hits' prefix counts scanned four hits at a time in rows of sixteen lanes and the
  second state of a pair counted from the first: -> 2.63; `postings_kernel`'s contig from a per-block table instead of a search: 19.2 -> 18.1 ms; the host's
  fragment bookkeeping done while the minimizer kernel runs and its k-dependent tables made once per context: -6 ms per run.

'''
r = P / "README.md"
t = r.read_text()
a = t.index("## Round 6\n")
b = t.index("## Round 5\n")
r.write_text(t[:a] + text + t[b:])
print("profiles/README.md: round 6 section rewritten")
