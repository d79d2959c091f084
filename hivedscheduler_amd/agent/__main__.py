"""Node health agent entry point:
`python -m hivedscheduler_amd.agent --scheduler http://hived:9096`."""
import argparse
import logging


def main() -> None:
    ap = argparse.ArgumentParser(prog="hivedscheduler-amd-agent")
    ap.add_argument("--scheduler", default=None, help="scheduler base URL")
    ap.add_argument("--local", action="store_true",
                    help="one local health sweep (deep + sweep), print JSON, no posting")
    ap.add_argument("--node-name", default=None)
    ap.add_argument("--interval", type=float, default=60.0)
    ap.add_argument("--deep-every", type=int, default=10,
                    help="run HIP kernel probes every N sweeps")
    # pair probes default ON (the xGMI checks are the point of the agent)
    ap.add_argument("--probe-pairs", action="store_true", default=True)
    ap.add_argument("--no-probe-pairs", dest="probe_pairs", action="store_false",
                    help="skip the RCCL xGMI pair probes during deep sweeps")
    ap.add_argument("--p2p-matrix-every", type=int, default=30,
                    help="full 28-pair p2p link-matrix sweep every N deep sweeps")
    ap.add_argument("--p2p-matrix", action="store_true",
                    help="with --local: also measure the full p2p link matrix")
    ap.add_argument("--burn-every", type=int, default=0,
                    help="sustained MFMA burn-in every N sweeps (on deep sweeps); 0 = never")
    ap.add_argument("--min-mfma-tflops", type=float, default=None,
                    help="mark a GPU bad when its burn-in bf16 TFLOP/s is below this "
                         "(no default: measure your fleet, see docs/user-manual.md)")
    ap.add_argument("--burn", action="store_true",
                    help="with --local: also run the MFMA burn-in")
    ap.add_argument("--lds-march-every", type=int, default=0,
                    help="full-LDS march (160 KiB per CU, both polarities) every N sweeps "
                         "(on deep sweeps); 0 = never")
    ap.add_argument("--lds-march", action="store_true",
                    help="with --local: also run the full-LDS march")
    ap.add_argument("--hbm-march-every", type=int, default=0,
                    help="HBM march (both polarities, fault location, per-XCD bandwidth; "
                         "holds up to 16 GiB) every N sweeps (on deep sweeps); 0 = never")
    ap.add_argument("--hbm-march", action="store_true",
                    help="with --local: also run the HBM march")
    ap.add_argument("--min-xcd-ratio", type=float, default=None,
                    help="mark a GPU bad when one XCD's march read rate is below this "
                         "fraction of the median XCD (no default: measure your fleet, see "
                         "docs/user-manual.md)")
    ap.add_argument("--simd-probe-every", type=int, default=0,
                    help="SIMD probe (exact VALU burn and register-file march, per-SIMD "
                         "attribution) every N sweeps (on deep sweeps); 0 = never")
    ap.add_argument("--simd-probe", action="store_true",
                    help="with --local: also run the SIMD probe")
    ap.add_argument("--scalar-probe-every", type=int, default=0,
                    help="scalar probe (exact SALU burn, SGPR march, scalar-load check, "
                         "per-SIMD attribution) every N sweeps (on deep sweeps); 0 = never")
    ap.add_argument("--scalar-probe", action="store_true",
                    help="with --local: also run the scalar probe")
    ap.add_argument("--atomic-probe-every", type=int, default=0,
                    help="atomic probe (exact atomic burn per CU, contended ticket / reduce / "
                         "cmpswap across all XCDs) every N sweeps (on deep sweeps); 0 = never")
    ap.add_argument("--atomic-probe", action="store_true",
                    help="with --local: also run the atomic probe")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    logging.basicConfig(level=logging.INFO)

    from .health import NodeHealthAgent, collect_node_health, p2p_link_matrix

    if args.local:
        import json

        report = collect_node_health(deep=True, sweep=True,
                                     probe_pairs=args.probe_pairs, burn=args.burn,
                                     min_mfma_tflops=args.min_mfma_tflops,
                                     lds_march=args.lds_march, hbm_march=args.hbm_march,
                                     min_xcd_ratio=args.min_xcd_ratio,
                                     simd_probe=args.simd_probe,
                                     scalar_probe=args.scalar_probe,
                                     atomic_probe=args.atomic_probe)
        if args.p2p_matrix:
            try:
                m = p2p_link_matrix()
                report["p2p_matrix"] = m["matrix"]
                if m["links"]:
                    report["links"] = m["links"]
            except Exception as e:
                report["p2p_matrix_error"] = str(e)[:200]
        print(json.dumps(report, indent=2))
        return
    if not args.scheduler:
        ap.error("--scheduler is required (or use --local)")
    agent = NodeHealthAgent(args.scheduler, node_name=args.node_name,
                            interval_s=args.interval, deep_every=args.deep_every,
                            probe_pairs=args.probe_pairs,
                            p2p_matrix_every=args.p2p_matrix_every,
                            burn_every=args.burn_every,
                            min_mfma_tflops=args.min_mfma_tflops,
                            lds_march_every=args.lds_march_every,
                            hbm_march_every=args.hbm_march_every,
                            min_xcd_ratio=args.min_xcd_ratio,
                            simd_probe_every=args.simd_probe_every,
                            scalar_probe_every=args.scalar_probe_every,
                            atomic_probe_every=args.atomic_probe_every)
    if args.once:
        import json

        print(json.dumps(agent.run_once(), indent=2))
    else:
        agent.run_forever()


if __name__ == "__main__":
    main()
