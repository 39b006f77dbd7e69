# experiments on kbo_map_batch_dev at C2: anchors on the 15-base table (seeds + present windows)
for A in 0 1; do echo "ANCHORS=$A: $(CHECK=0 KBO_DEPTH_TABLE_ANCHORS=$A python tools/exp_map.py 2>&1 | tail -1)"; done
