package gpuaoi

// Batched reads of the interest sets (gw_set_tags, gw_neighbors_batch,
// gw_nearest, gw_related): what game logic pulls from InterestedIn per entity
// per timer (examples/unity_demo/Monster.go:48-98), asked once per timer
// period for all the entities of a space.  Every query sees the state of the
// last Flush: calls buffered since then are invisible, and an entity that has
// entered no space yet (or only since the last Flush) has an empty set.
// Uncompiled, as the rest of the shim (no Go toolchain where it was written);
// tests/test_gpu_queries.py makes the same calls through the same ABI.

/*
#include "gpuaoi.h"
*/
import "C"

import (
	"math"
	"unsafe"

	"github.com/xiaonanln/go-aoi"
	"github.com/xiaonanln/goworld/engine/gwlog"
)

// NoSlot: gw_nearest_rec.slot when nobody matches.
const NoSlot uint32 = C.GW_NO_SLOT

// SetTag sets the entity's 32-bit query tag: opaque to the library, e.g. a
// type id in the low bits and an "alive" bit (Monster.AI's TypeName and hp
// tests, Monster.go:52-58).  A query's (mask, value) keeps the related
// entities whose (tag & mask) == value.  Buffered like the ids: applied to the
// entity's slot with them, and again whenever take() hands it a slot.
func (c *Context) SetTag(a *aoi.AOI, tag uint32) {
	c.info(a).tag = tag
	c.idDirty[a] = true
}

// querySlot: the slot whose state the library holds for a, if any.
func (c *Context) querySlot(a *aoi.AOI) (uint32, bool) {
	m := c.cur[a]
	if m == nil {
		return 0, false
	}
	s, ok := m.slotOf[a]
	if !ok || m.parked[a] {
		return 0, false
	}
	return s, true
}

// querySlots: the slots of ents that have one, and for each the index it came from.
func (c *Context) querySlots(ents []*aoi.AOI) (slots []C.uint32_t, from []int) {
	c.applyIDs() // tags set since the last submit
	for i, a := range ents {
		if s, ok := c.querySlot(a); ok {
			slots = append(slots, C.uint32_t(s))
			from = append(from, i)
		}
	}
	return
}

// NeighborsBatch is InterestedIn of every ents[k] filtered by tag, in one
// call: out[k] lists the matching related entities in ascending slot order
// (nil for an entity outside every space).  mask = value = 0 keeps everyone.
func (c *Context) NeighborsBatch(ents []*aoi.AOI, tagMask, tagValue uint32) [][]*aoi.AOI {
	out := make([][]*aoi.AOI, len(ents))
	slots, from := c.querySlots(ents)
	if len(slots) == 0 {
		return out
	}
	var no C.gw_nbr_out
	c.check(C.gw_neighbors_batch(c.ctx, &slots[0], C.uint32_t(len(slots)), C.uint32_t(tagMask), C.uint32_t(tagValue),
		C.GW_QUERY_COPY_TO_HOST, &no))
	off := unsafe.Slice(no.off, len(slots)+1)
	var nbr []C.uint32_t
	if no.n_nbr > 0 {
		nbr = unsafe.Slice(no.nbr, int(no.n_nbr))
	}
	for k, i := range from {
		l := make([]*aoi.AOI, 0, int(off[k+1]-off[k]))
		for _, w := range nbr[off[k]:off[k+1]] {
			l = append(l, c.aoiOf[w])
		}
		out[i] = l
	}
	return out
}

// NearestResult: Monster.AI's answer for one entity.
type NearestResult struct {
	Target *aoi.AOI // the matching related entity nearest to it; nil when nobody matches
	Count  uint32   // matching related entities
	Dist   float32  // Entity.DistanceTo(Target) (Vector3.go:23-28: float32, Y included); +Inf when nobody matches
}

// Nearest is Monster.AI's loop over InterestedIn (Monster.go:48-76) for every
// ents[k] in one launch: the related entity with (tag & mask) == value at the
// smallest Entity.DistanceTo, positions as of the last Flush.  Among entities
// at equal distance the reference keeps whichever Go's map iteration met
// first; here it is the one in the lowest slot.
func (c *Context) Nearest(ents []*aoi.AOI, tagMask, tagValue uint32) []NearestResult {
	out := make([]NearestResult, len(ents))
	for i := range out {
		out[i].Dist = float32(math.Inf(1)) // an entity outside every space: nobody
	}
	slots, from := c.querySlots(ents)
	if len(slots) > 0 {
		var no C.gw_near_out
		c.check(C.gw_nearest(c.ctx, &slots[0], C.uint32_t(len(slots)), C.uint32_t(tagMask), C.uint32_t(tagValue),
			C.GW_QUERY_COPY_TO_HOST, &no))
		for k, r := range unsafe.Slice(no.rec, len(slots)) {
			res := NearestResult{Count: uint32(r.count), Dist: float32(r.dist)}
			if uint32(r.slot) != NoSlot {
				res.Target = c.aoiOf[r.slot]
			}
			out[from[k]] = res
		}
	}
	return out
}

// Related is Entity.IsInterestedIn (Entity.go:249-251; Monster.Tick,
// Monster.go:79,89) for the pairs (a[i], b[i]) in one call.
func (c *Context) Related(a, b []*aoi.AOI) []bool {
	if len(a) != len(b) {
		gwlog.Panicf("gpuaoi: Related with %d a and %d b", len(a), len(b))
	}
	out := make([]bool, len(a))
	var sa, sb []C.uint32_t
	var from []int
	for i := range a {
		x, okx := c.querySlot(a[i])
		y, oky := c.querySlot(b[i])
		if okx && oky {
			sa, sb, from = append(sa, C.uint32_t(x)), append(sb, C.uint32_t(y)), append(from, i)
		}
	}
	if len(sa) == 0 {
		return out
	}
	res := make([]C.uint8_t, len(sa))
	c.check(C.gw_related(c.ctx, &sa[0], &sb[0], C.uint32_t(len(sa)), &res[0]))
	for k, i := range from {
		out[i] = res[k] != 0
	}
	return out
}
