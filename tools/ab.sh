#!/bin/bash
# Same-box A/B of two builds of libpanmap_amd.so (GPU boxes differ by ~5 %): copy the builds to build_variants/ and run
#   tools/ab.sh base.so new.so      -> alternating bench.py runs, M reads/s, ms/step, the dominant align kernel and the align stage (ms)
# A variant may name one `ab` switch to set for its runs, lib.so:SWITCH -- one build with and without a design decision:
#   tools/ab.sh new.so new.so:PMX_ALIGN_NO_NEAR      (the compact tier's class lists without the near class)
cd "$(dirname "$0")/.."
for r in 1 2 3; do for v in "$@"; do
  lib=${v%%:*}; sw=; [ "$lib" != "$v" ] && sw="${v#*:}=1"
  env $sw PMX_LIB_PATH=$PWD/build_variants/$lib timeout 600 python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline 2>&1 | tail -1 | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); k=d['kernels_ms']; print('$v', round(d['value']/1e6,2), round(d['ms_per_step'],2), 'dominant', round(k['dominant align kernel'],2), 'align', round(k['align stage (all tiers)'],2))"
done; done
