# fp8 mode A/B on one box: activation quantisation on/off, fused down+qkv launch on/off: engine options
# fp8_decode_act / decode_fuse (the library reads no environment variable)
timeout 600 python -m pytest tests/test_gpu_parity.py -q -x -k "fp8 or fused" 2>&1 | tail -5
for cfg in "1 1" "1 0" "0 1"; do
  set -- $cfg
  timeout 300 python bench.py --option fp8_decode_act=$1 --option decode_fuse=$2 --steps 5 --warmup 2 --precision fp8 --no-cpu-baseline --no-b64 --inflight 0 --no-alt-modes 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('act $1 fuse $2 B32', d['value'], d['phase_ms'])"
  timeout 300 python bench.py --option fp8_decode_act=$1 --option decode_fuse=$2 --steps 3 --warmup 1 --preset configs4 --no-cpu-baseline --no-b64 --inflight 0 --no-alt-modes 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('act $1 fuse $2 B128', d['value'], d['phase_ms'])"
done
