#!/bin/bash
# Register / scratch / LDS usage of every kernel as hipcc reports it (-Rpass-analysis=kernel-resource-usage), one line per
# kernel -> profiles/${ROUND}_kernel_resource_usage.txt.  Compiles what csrc/Makefile compiles -- its SRCS with its CXXFLAGS, and the
# two files it builds once more for fp16 storage (rows marked [f16]).  Runs on the build container (cross-compiles, no GPU).
# ONLY=head_mfma.hip restricts it to one file.
ROUND=${ROUND:-r04}
cd "$(dirname "$0")/../torch-mednet_amd/csrc" || exit 1
OUT=../../profiles/${ROUND}_kernel_resource_usage.txt
ARCH=gfx950
FLAGS=$(sed -n 's/^CXXFLAGS *= *//p' Makefile | sed "s/\$(ARCH)/$ARCH/")
SRCS=${ONLY:-$(sed -n 's/^SRCS *= *//p' Makefile)}
F16=$(sed -n 's/^OBJS *= *//p' Makefile | tr ' ' '\n' | sed -n 's/_f16\.o$/.hip/p' | tr '\n' ' ')
F16FLAGS=$(sed -n 's/.*\$(CXXFLAGS) \(-DMEDNET_ELT_F16[^$]*\) -c.*/\1/p' Makefile)
TMP=$(mktemp -d)
echo "# hipcc $FLAGS -Rpass-analysis=kernel-resource-usage, $(git rev-parse --short HEAD 2>/dev/null)" > $OUT
usage() {  # file, tag, extra flags
  /opt/rocm/bin/hipcc $FLAGS $3 -Rpass-analysis=kernel-resource-usage -c $1 -o $TMP/ru.o 2>&1 |
  TAG="$1$2" python3 -c "
import os,re,sys,subprocess
tag=os.environ['TAG']
txt=sys.stdin.read().split('Function Name: ')[1:]
for t in txt:
    name=t.split(' ')[0]
    g=lambda k: (re.search(k+r'[^:\n]*: (\d+)',t) or [0,'?'])[1]
    dem=subprocess.run(['c++filt',name],capture_output=True,text=True).stdout.strip()
    dem=re.sub(r'\(.*','',dem)[:70]
    print(f'{tag}  {dem:70s} VGPRs={g(\"VGPRs\")} AGPRs={g(\"AGPRs\")} SGPRs={g(\"SGPRs\")} ScratchSize={g(\"ScratchSize\")} VGPRSpill={g(\"VGPRs Spill\")} Occupancy={g(\"Occupancy\")} LDS={g(\"LDS Size\")}')
" >> $OUT
}
for f in $SRCS; do
  usage $f "" ""
  case " $F16 " in *" $f "*) usage $f "[f16]" "$F16FLAGS" ;; esac
done
rm -rf $TMP
grep -c . $OUT; awk '{for(i=1;i<=NF;i++) if ($i ~ /^ScratchSize=/ && $i != "ScratchSize=0") print}' $OUT
