package yoda

// The split refresh() makes of changed SCV records, no GPU needed:
//
//	go test ./pkg/yoda/ -run RecordDelta
//
// NOT COMPILED HERE (no Go toolchain in the build image); see INTEGRATION.md.

import (
	"testing"

	scv "github.com/NJUPT-ISL/SCV/api/v1"
)

// The split refresh() makes of two SCV records of one node: a static change (ReplaceNodes) wins
// over a dynamic one (UpdateCards); equal records are neither.
func TestRecordDelta(t *testing.T) {
	rec := func() *scv.Scv {
		s := &scv.Scv{}
		s.Status.CardNumber, s.Status.FreeMemorySum, s.Status.TotalMemorySum = 2, 300, 1000
		s.Status.CardList = []scv.Card{
			{Health: "Healthy", FreeMemory: 100, TotalMemory: 500, Clock: 1500, Bandwidth: 900, Core: 80, Power: 300},
			{Health: "Healthy", FreeMemory: 200, TotalMemory: 500, Clock: 1500, Bandwidth: 900, Core: 80, Power: 300}}
		return s
	}
	a := rec()
	if staticChanged(a, rec()) || dynamicChanged(a, rec()) {
		t.Fatal("equal records differ")
	}
	b := rec()
	b.Status.CardList[1].FreeMemory, b.Status.FreeMemorySum = 150, 250
	if staticChanged(a, b) || !dynamicChanged(a, b) {
		t.Error("a new FreeMemory is a card update")
	}
	b = rec()
	b.Status.CardList[0].Health = "Unhealthy"
	if staticChanged(a, b) || !dynamicChanged(a, b) {
		t.Error("a new Health is a card update")
	}
	for name, change := range map[string]func(*scv.Scv){
		"clock":      func(s *scv.Scv) { s.Status.CardList[1].Clock = 1755 },
		"total":      func(s *scv.Scv) { s.Status.CardList[0].TotalMemory = 600 },
		"totalSum":   func(s *scv.Scv) { s.Status.TotalMemorySum = 1100 },
		"cardNumber": func(s *scv.Scv) { s.Status.CardNumber = 1 },
		"cards":      func(s *scv.Scv) { s.Status.CardList = s.Status.CardList[:1] },
	} {
		b = rec()
		change(b)
		if !staticChanged(a, b) {
			t.Errorf("%s: a static change goes to ReplaceNodes", name)
		}
	}
	if !sameNames([]string{"a", "b"}, []string{"a", "b"}) || sameNames([]string{"a"}, []string{"b"}) ||
		sameNames([]string{"a"}, []string{"a", "b"}) {
		t.Error("sameNames")
	}
}
