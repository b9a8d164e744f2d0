package gpuaoi

// The batched queries through the shim, on a hand-made space (the cases of
// tests/test_gpu_queries.py::test_known_answers_through_the_abi and
// test_tags_lifecycle): lists, nearest with a tag filter and Y in the
// distance, pairs, visibility (the state of the last Flush) and a tag that
// stays with its entity across Leave and Enter.  Needs the MI355X.

import (
	"math"
	"testing"

	"github.com/xiaonanln/go-aoi"
	"github.com/xiaonanln/goworld/engine/proto"
)

const (
	tagPlayer  uint32 = 1
	tagMonster uint32 = 2
	tagAlive   uint32 = 0x100
)

func queryEntity(id uint32, d aoi.Coord, log *[2][]event) *testEntity {
	e := &testEntity{id: id, log: log}
	aoi.InitAOI(&e.a, d, e, e)
	return e
}

func TestQueries(t *testing.T) {
	c := NewContext(0)
	defer c.Close()
	m := c.NewManager(100, 8, -1000, -1000, 1000, 1000)
	var log [2][]event
	pos := [][3]float32{{0, 0, 0}, {1, 1000, 1}, {50, 0, 50}, {400, 0, 0}, {403, 0, 4}}
	tags := []uint32{tagMonster | tagAlive, tagPlayer | tagAlive, tagPlayer | tagAlive, tagMonster | tagAlive, tagPlayer}
	var es []*testEntity
	var as []*aoi.AOI
	for i, p := range pos {
		e := queryEntity(uint32(i), 100, &log)
		e.pos = proto.EntitySyncInfo{X: p[0], Y: p[1], Z: p[2]}
		c.SetTag(&e.a, tags[i]) // before Enter
		m.EnterPos(&e.a, p[0], p[1], p[2], 0)
		es, as = append(es, e), append(as, &e.a)
	}
	// nothing flushed yet: every set is empty
	for k, l := range c.NeighborsBatch(as, 0, 0) {
		if len(l) != 0 {
			t.Fatalf("entity %d has neighbours before the first Flush", k)
		}
	}
	c.Flush()
	ids := func(l []*aoi.AOI) (out []uint32) {
		for _, a := range l {
			out = append(out, a.Data.(*testEntity).id)
		}
		return
	}
	want := [][]uint32{{1, 2}, {0, 2}, {0, 1}, {4}, {3}}
	for k, l := range c.NeighborsBatch(as, 0, 0) {
		got := ids(l)
		if len(got) != len(want[k]) {
			t.Fatalf("list %d: %v, want %v", k, got, want[k])
		}
		for i := range got {
			if got[i] != want[k][i] {
				t.Fatalf("list %d: %v, want %v", k, got, want[k])
			}
		}
	}
	// Monster.AI: the nearest live Player.  (1, 1000, 1) is in the set but Y counts.
	r := c.Nearest(as[:1], 0xff|tagAlive, tagPlayer|tagAlive)[0]
	if r.Target != as[2] || r.Count != 2 || r.Dist != float32(math.Sqrt(5000)) {
		t.Fatalf("nearest live player of 0: %+v", r)
	}
	// entity 3's only neighbour is a dead Player: nobody matches
	r = c.Nearest(as[3:4], 0xff|tagAlive, tagPlayer|tagAlive)[0]
	if r.Target != nil || r.Count != 0 || !math.IsInf(float64(r.Dist), 1) {
		t.Fatalf("nearest live player of 3: %+v", r)
	}
	r = c.Nearest(as[3:4], 0, 0)[0]
	if r.Target != as[4] || r.Dist != 5 {
		t.Fatalf("nearest of 3: %+v", r)
	}
	// Monster.Tick: IsInterestedIn(target)
	rel := c.Related([]*aoi.AOI{as[0], as[0], as[3], as[0]}, []*aoi.AOI{as[2], as[3], as[4], as[0]})
	if !rel[0] || rel[1] || !rel[2] || rel[3] {
		t.Fatalf("related: %v", rel)
	}
	// a move is invisible until the Flush
	es[3].pos.X = 10
	m.MovedPos(as[3], 10, 0, 0, 0, SifOwnClient|SifNeighborClients)
	if c.Related(as[:1], as[3:4])[0] {
		t.Fatal("a buffered move is visible")
	}
	c.Flush()
	if !c.Related(as[:1], as[3:4])[0] {
		t.Fatal("the flushed move is not visible")
	}
	// the tag stays with the entity across Leave and Enter (a new slot or the same)
	m.LeaveKeep(as[2], 0)
	c.Flush()
	m.EnterPos(as[2], 20, 0, 0, 0)
	c.Flush()
	r = c.Nearest(as[:1], 0xff|tagAlive, tagPlayer|tagAlive)[0]
	if r.Target != as[2] || r.Dist != 20 {
		t.Fatalf("nearest live player of 0 after the re-Enter: %+v", r)
	}
	// the player dies: one SetTag, seen by the next query
	c.SetTag(as[2], tagPlayer)
	r = c.Nearest(as[:1], 0xff|tagAlive, tagPlayer|tagAlive)[0]
	if r.Target != as[1] || r.Count != 1 {
		t.Fatalf("nearest live player of 0 after 2 died: %+v", r)
	}
}
