#!/bin/bash
# tools/ab_env.sh "<VAR=value ...>" ... : the bench's timed region under different environment settings (quoted groups),
# alternating, three rounds, inside one GPU lease.  An empty group "" is the default configuration.
one() { env "$@" python bench.py --full --no-cpu-baseline --no-extras --steps 60 --warmup 10 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['roofline']['kernel'], d['roofline']['isolated']['achieved'])"; }
for rep in 1 2 3; do for g in "$@"; do echo "[$g] $(one $g)"; done; done
