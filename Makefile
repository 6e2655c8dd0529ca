# Convenience targets; the driver's contract is __graft_entry__.build()/smoke() and bench.py.
.PHONY: build test test-gpu bench smoke example place bridge crank piston snap rest wind fold marbles fit reach logs ramp bullet clean

build:                      ## hipcc --offload-arch=gfx950 -> phyx_amd/libphyx_amd.so; gcc -> oracle/liboracle.so (+ oracle/_ref shims if /root/reference exists)
	python -c "import __graft_entry__ as g; g.build()"

test: build                 ## CPU suite (no GPU needed)
	python -m pytest tests -q -m "not gpu"

test-gpu: build             ## parity suite on an MI355X
	python -m pytest tests -q -m gpu

smoke: build
	python __graft_entry__.py --smoke

bench: build
	python bench.py

example: build              ## the C ABI from plain C
	gcc -std=c11 -O2 -Wall -Iinclude examples/drop_in.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -o examples/drop_in

place: build                ## the emitter that looks first (phx_world_query_boxes, phx_world_cast_boxes)
	gcc -std=c11 -O2 -Wall -Iinclude examples/place.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/place

bridge: build               ## links: a pinned deck on rod hangers, a crate on a rope, a box on a spring (phx_world_add_links)
	gcc -std=c11 -O2 -Wall -Iinclude examples/bridge.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/bridge

crank: build                ## angles: a door with stops, a wheel on a motor, two boxes welded by a pin plus a lock (phx_world_add_angles)
	gcc -std=c11 -O2 -Wall -Iinclude examples/crank.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/crank

piston: build               ## sliders: a crank-slider, an elevator between its stops, a box on a spring slider (phx_world_add_sliders)
	gcc -std=c11 -O2 -Wall -Iinclude examples/piston.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/piston

snap: build                 ## breaks: the bridge's hangers under a limit, crates dropped until they snap (phx_world_set_break_limits, phx_world_break_events)
	gcc -std=c11 -O2 -Wall -Iinclude examples/snap.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/snap

rest: build                 ## sleeping: boxes drop onto a shelf until the pile rests, a crate wakes the column it hits (phx_world_set_sleeping)
	gcc -std=c11 -O2 -Wall -Iinclude examples/rest.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/rest

wind: build                 ## force fields: boxes drop through a wind zone into a drag pool, a blast scatters the pile (phx_world_set_fields, phx_world_pulse_fields)
	gcc -std=c11 -O2 -Wall -Iinclude examples/wind.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/wind

fold: build                 ## collision exclusions: a folded chain dropped on its end, once with one negative group, once with its neighbours excluded (phx_world_add_collision_exclusions)
	gcc -std=c11 -O2 -Wall -Iinclude examples/fold.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/fold

logs: build                 ## shapes: a dozen capsules dropped onto a shelf between two posts, one that topples from its end (PHX_SHAPE_CAPSULE)
	gcc -std=c11 -O2 -Wall -Iinclude examples/logs.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/logs

ramp: build                 ## shapes: boxes slide, marbles roll and a hexagon tumbles down a static wedge into a trapezoid tray; a ray onto the slope (PHX_SHAPE_POLYGON, phx_world_set_polygons)
	gcc -std=c11 -O2 -Wall -Iinclude examples/ramp.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/ramp

bullet: build               ## continuous bodies: marbles at 120 units/s against a thin wall and ramp's wedge, once discrete (they tunnel) and once continuous (phx_world_set_continuous, phx_world_sweep_hits)
	gcc -std=c11 -O2 -Wall -Iinclude examples/bullet.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/bullet

marbles: build              ## shapes: circles dropped through a funnel of static boxes into a tray, a round wheel on a motor (phx_world_set_shapes)
	gcc -std=c11 -O2 -Wall -Iinclude examples/marbles.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/marbles

fit: build                  ## the marble emitter that looks first (phx_world_query_circles, phx_world_cast_circles)
	gcc -std=c11 -O2 -Wall -Iinclude examples/fit.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/fit

reach: build                ## a pick with a tolerance and the marbles' clearance from the funnel (phx_world_query_nearest)
	gcc -std=c11 -O2 -Wall -Iinclude examples/reach.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$(CURDIR)/phyx_amd -lm -o examples/reach

clean:
	rm -f phyx_amd/libphyx_amd.so oracle/liboracle.so examples/drop_in examples/place examples/bridge examples/crank examples/piston examples/snap examples/rest examples/wind examples/fold examples/marbles examples/fit examples/reach examples/logs examples/ramp examples/bullet
	rm -rf oracle/_ref
