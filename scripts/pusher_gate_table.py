"""Measures the CPU oracle against tests/pusher_model.py over the whole grid of regimes and prints
 * the literal GATES table of tests/pusher_model.py (the rule: pusher_model.gate_from), and
 * the markdown table of the oracle's worst err_ulp per cell (profiles/round11/README.md).

    python scripts/pusher_gate_table.py            # oracle (CPU)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import pusher_model as M  # noqa: E402
from tests.oracle_lib import load_oracle  # noqa: E402


def main():
    oracle = load_oracle()
    worst = {}
    for pusher in M.PUSHERS:
        for fields in M.ALL_FIELD_SETS:
            for u_over_c in M.U_OVER_C:
                w = 0.0
                for species in M.SPECIES:
                    parts, E, B, q, m, dt, _ = M.launch_inputs(fields, species, u_over_c)
                    got = M.oracle_push(oracle, pusher, parts, E, B, q, m, dt, 0)
                    err, _ = M.judge(got, pusher, fields, species, u_over_c, 0, 0)
                    w = max(w, float(err.max()))
                worst[pusher, fields, u_over_c] = w
    print("GATES = {")
    for pusher in M.PUSHERS:
        print(f'    "{pusher}": {{')
        for fields in M.ALL_FIELD_SETS:
            if (pusher, fields) in M.REPORTED:
                continue
            gates = ", ".join(str(M.gate_from(worst[pusher, fields, u])) for u in M.U_OVER_C)
            print(f'        "{fields}": ({gates}),')
        print("    },")
    print("}\n")
    print("| pusher | field set | " + " | ".join(f"u/c = {u:g}" for u in M.U_OVER_C) + " |")
    print("|---|---|" + "---|" * len(M.U_OVER_C))
    for pusher in M.PUSHERS:
        for fields in M.ALL_FIELD_SETS:
            tag = " (reported)" if (pusher, fields) in M.REPORTED else ""
            print(f"| {pusher} | {fields}{tag} | " + " | ".join(f"{worst[pusher, fields, u]:.3g}" for u in M.U_OVER_C) + " |")


if __name__ == "__main__":
    main()
